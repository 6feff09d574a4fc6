// qe_csv_device.hip -- the kernels of the device CSV parser (host side: qe_csv_device.cpp).
//
//   1. quote counts per 4 KiB tile; their exclusive scan (the host's) is the quote parity at every tile start;
//   2. one wave per tile walks its bytes 64 at a time: a ballot of the quotes gives the parity before every byte, so the
//      line ends outside quotes, and with them the starts of the non-empty records, are known byte-parallel.  The same pass
//      proves that every '"' is the enclosing quote of a field -- an opening quote (even parity) follows the text start,
//      ',', '\n', '\r' or '"', a closing one (odd parity) precedes the text end, ',', '\n', '\r' or '"' -- which is exactly
//      when quote parity equals the sequential state machine of next_record.  A count pass, a scan, then a write pass
//      that stores the record starts in row order;
//   3. one thread per record walks its fields and notes the span of every projected one;
//   4. one thread per row and column converts: DOUBLE through qe_csv_number.h (fields it leaves undecided go to a patch
//      list the host converts), BOOLEAN, validity -- bitmaps as one ballot per 64 rows; STRING fields are hashed, inserted
//      into an open-addressing table (bytes compared on a hash match) and numbered by their first row (a scan over the rows
//      that are the first of their string);
//   5. the unescaped bytes of the fields of a row list, packed back to back: the distinct strings for the host's dictionary,
//      the patch list for the host's converter.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "qe_csv_number.h"
#include "qe_kernels.h"
#include "qe_scan.h"

namespace qe {
namespace {

constexpr u32 kEmpty = 0xFFFFFFFFu;

__device__ inline bool is_sep(unsigned char c) { return c == ',' || c == '\n' || c == '\r' || c == '"'; }

inline unsigned grid_of(i64 n, i64 per) { return (unsigned)std::max<i64>(1, (n + per - 1) / per); }

// the structure passes: four waves a block, one tile each
struct WaveTile { i64 tile; int lane; };
__device__ inline WaveTile wave_tile() { return {(i64)blockIdx.x * 4 + (threadIdx.x >> 6), (int)(threadIdx.x & 63)}; }
// the passes that ballot a bitmap word: 64 consecutive rows a wave, from row r0 on; this lane's row is r (maybe past the last)
struct WaveRows { i64 r0, r; };
__device__ inline WaveRows wave_rows() {
    const i64 r0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63);
    return {r0, r0 + (threadIdx.x & 63)};
}

// ---- 1. quotes per tile ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) quote_count_kernel(const unsigned char *text, i64 ntiles, i64 *tile_quotes) {
    const auto [tile, lane] = wave_tile();
    if (tile >= ntiles) return;
    // the text buffer is padded with zero bytes to whole tiles: every lane reads its 64 bytes unguarded
    const uint4 *p = (const uint4 *)(text + tile * kCsvTile + lane * 64);
    int cnt = 0;
    for (int k = 0; k < 4; k++) {
        const uint4 q = p[k];
        const u32 words[4] = {q.x, q.y, q.z, q.w};
        for (int j = 0; j < 4; j++) {
            const u32 y = words[j] ^ 0x22222222u;                  // a '"' byte becomes zero
            const u32 t = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);   // 0x80 exactly at the zero bytes
            cnt += __popc(t);
        }
    }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if (lane == 0) tile_quotes[tile] = cnt;
}

// ---- 2. record starts ------------------------------------------------------------------------------------------------
// WRITE = false: count the non-empty record starts of every tile and check the quote rule; true: store them at their row.
template <bool WRITE>
__global__ void __launch_bounds__(256) records_kernel(const unsigned char *text, i64 n, i64 ntiles, const i64 *tile_quotes_before,
                                                      i64 *tile_rows, i64 *rec_start, u32 *flags) {
    const auto [tile, lane] = wave_tile();
    if (tile >= ntiles) return;
    const u64 lt = (1ull << lane) - 1;
    const i64 base = tile * kCsvTile;
    u32 parity = (u32)(tile_quotes_before[tile] & 1);
    unsigned char carry_prev = base > 0 ? text[base - 1] : 0;   // the byte in front of this step's lane 0
    i64 out = WRITE ? tile_rows[tile] : 0;
    i64 count = 0;
    bool bad = false;
    for (int s = 0; s < kCsvTile / 64; s++) {
        const i64 i = base + s * 64 + lane;
        const unsigned char c = i < n ? text[i] : 0;
        unsigned char prev = (unsigned char)wave_prev((int)c);
        if (lane == 0) prev = carry_prev;
        carry_prev = (unsigned char)__shfl((int)c, 63, 64);
        const u64 qm = __ballot(c == '"');
        const u32 inq = parity ^ (u32)(__popcll(qm & lt) & 1);   // quote parity before byte i
        parity ^= (u32)(__popcll(qm) & 1);
        if (!WRITE && c == '"' && i < n) {
            if (inq == 0) bad |= !(i == 0 || is_sep(prev));                         // opening quote
            else bad |= !(i + 1 == n || is_sep(text[i + 1]));                        // closing quote
        }
        // a record starts at i when i is the text start or follows a line end outside quotes (\r\n counts at its \n)
        const bool start = i < n && inq == 0 && (i == 0 || prev == '\n' || (prev == '\r' && c != '\n'));
        const bool row = start && c != '\n' && c != '\r';                       // empty lines are skipped
        const u64 rm = __ballot(row);
        if (WRITE && row) rec_start[out + count + __popcll(rm & lt)] = i;
        count += __popcll(rm);
    }
    if (!WRITE) {
        if (__any(bad) && lane == 0) atomicOr(flags, (u32)QE_CSV_QUOTE_RULE);
        if (lane == 0) tile_rows[tile] = count;
    }
}

// ---- 3. field spans --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) spans_kernel(const CsvSpanArgs a) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 nrows = a.all.nrows;
    if (r >= nrows) return;
    for (int k = 0; k < a.ncols; k++) { a.all.begin[k * nrows + r] = 0; a.all.lenesc[k * nrows + r] = 0; }
    const unsigned char *t = a.all.text;
    i64 pos = a.rec_start[r];
    for (int f = 0; f <= a.max_field; f++) {
        i64 cb, ce;
        u32 esc = 0;
        if (pos < a.n && t[pos] == '"') {   // enclosed: the structure pass proved that a lone '"' closes it
            cb = ++pos;
            for (; pos < a.n;) {   // (the bound only guards: a closing quote exists)
                if (t[pos] == '"') {
                    if (pos + 1 < a.n && t[pos + 1] == '"') { esc = 1; pos += 2; continue; }
                    break;
                }
                pos++;
            }
            ce = pos++;
        } else {
            cb = pos;
            while (pos < a.n && t[pos] != ',' && t[pos] != '\n' && t[pos] != '\r') pos++;
            ce = pos;
        }
        for (int k = 0; k < a.ncols; k++)
            if (a.field_of[k] == f) {
                a.all.begin[k * nrows + r] = cb;
                a.all.lenesc[k * nrows + r] = (u32)(ce - cb) << 1 | esc;
            }
        if (pos >= a.n || t[pos] != ',') break;   // the record ends; later fields are missing
        pos++;
    }
}

// The unescaped bytes of a field one at a time ("" -> ").
struct Unesc {
    const unsigned char *p;
    i64 i, end;
    bool esc;
    __device__ bool next(unsigned char &c) {
        if (i >= end) return false;
        c = p[i];
        i += (esc && c == '"') ? 2 : 1;
        return true;
    }
    __device__ i64 count() {   // the bytes that are left (consumes them)
        i64 len = 0;
        for (unsigned char c; next(c);) len++;
        return len;
    }
};
// .. of row r of a column
__device__ inline Unesc field_bytes(const CsvFields &f, i64 r) {
    const u32 le = f.lenesc[r];
    return Unesc{f.text, f.begin[r], f.begin[r] + (le >> 1), (le & 1) != 0};
}

// one 64-row word of a bitmap per wave; any_null is raised when a word misses a row that exists
__device__ inline void store_bits(u64 *words, u32 *any_null, const WaveRows &w, i64 nrows, bool value, bool valid, u64 *validity) {
    const u64 vb = __ballot(valid);
    const u64 bb = __ballot(value);
    if (w.r == w.r0 && w.r0 < nrows) {
        const i64 left = nrows - w.r0;
        const u64 full = left >= 64 ? ~0ull : ((1ull << left) - 1);
        if (words) words[w.r0 >> 6] = bb;
        validity[w.r0 >> 6] = vb;
        if (vb != full) atomicOr(any_null, 1u);
    }
}

// ---- 4a. DOUBLE / BOOLEAN --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) convert_double_kernel(const CsvConvArgs a) {
    const WaveRows w = wave_rows();
    const i64 r = w.r;
    bool valid = false;
    if (r < a.f.nrows) {
        const u32 le = a.f.lenesc[r];
        const u32 len = le >> 1;
        double v = 0.0;
        if (len > 0) {
            valid = true;
            if (le & 1) {
                atomicOr(a.flags, (u32)QE_CSV_BAD_NUMBER);   // a '"' inside: no Java literal
            } else {
                const int st = qe_parse_double(a.f.text + a.f.begin[r], len, v);
                if (st == QE_NUM_REJECT) {
                    atomicOr(a.flags, (u32)QE_CSV_BAD_NUMBER);
                } else if (st == QE_NUM_UNDECIDED) {
                    const u32 slot = atomicAdd(a.patch_count, 1u);
                    if (slot < a.patch_cap) a.patch_rows[slot] = r;
                    else atomicOr(a.flags, (u32)QE_CSV_PATCH_OVERFLOW);
                    v = 0.0;
                }
            }
        }
        ((double *)a.data)[r] = v;
    }
    store_bits(nullptr, a.any_null, w, a.f.nrows, false, valid, a.validity);
}

__global__ void __launch_bounds__(256) convert_bool_kernel(const CsvConvArgs a) {
    const WaveRows w = wave_rows();
    const i64 r = w.r;
    bool valid = false, value = false;
    if (r < a.f.nrows) {
        const u32 le = a.f.lenesc[r];
        valid = (le >> 1) > 0;
        if (le == (4u << 1)) {   // exactly four bytes, no escape: String.toBoolean
            const unsigned char *p = a.f.text + a.f.begin[r];
            value = (p[0] | 0x20) == 't' && (p[1] | 0x20) == 'r' && (p[2] | 0x20) == 'u' && (p[3] | 0x20) == 'e';
        }
    }
    store_bits((u64 *)a.data, a.any_null, w, a.f.nrows, value, valid, a.validity);
}

__global__ void __launch_bounds__(256) scatter_f64_kernel(double *data, const i64 *rows, const double *values, i64 n) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) data[rows[i]] = values[i];
}

// ---- 4b. STRING: device dictionary ------------------------------------------------------------------------------------
__device__ inline u64 mix64(u64 h) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 33);
}

__global__ void __launch_bounds__(256) dict_hash_kernel(const CsvDictArgs a) {
    const WaveRows w = wave_rows();
    const i64 r = w.r;
    bool valid = false;
    if (r < a.f.nrows) {
        valid = (a.f.lenesc[r] >> 1) > 0;
        u64 h = 0xcbf29ce484222325ull;
        Unesc u = field_bytes(a.f, r);
        unsigned char c;
        while (u.next(c)) h = (h ^ c) * 0x100000001b3ull;
        a.hash[r] = h;
    }
    store_bits(nullptr, a.any_null, w, a.f.nrows, false, valid, a.validity);
}

__device__ inline bool same_string(const CsvFields &f, i64 x, i64 y) {
    Unesc ux = field_bytes(f, x), uy = field_bytes(f, y);
    if (!ux.esc && !uy.esc && ux.end - ux.i != uy.end - uy.i) return false;
    for (;;) {
        unsigned char cx, cy;
        const bool hx = ux.next(cx), hy = uy.next(cy);
        if (hx != hy) return false;
        if (!hx) return true;
        if (cx != cy) return false;
    }
}

__global__ void __launch_bounds__(256) dict_insert_kernel(const CsvDictArgs a) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.f.nrows || (a.f.lenesc[r] >> 1) == 0) return;
    const u64 h = a.hash[r];
    u64 s = mix64(h) & a.mask;
    for (;;) {
        u32 cur = __hip_atomic_load(&a.slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty) {
            const u32 prev = atomicCAS(&a.slots[s], kEmpty, (u32)r);
            cur = prev == kEmpty ? (u32)r : prev;
        }
        if (cur == (u32)r || (a.hash[cur] == h && same_string(a.f, r, cur))) break;
        s = (s + 1) & a.mask;
    }
    a.row_slot[r] = (u32)s;
    // rows arrive roughly in order: most see a first row at or below their own and skip the atomic
    if (__hip_atomic_load(&a.first[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (u32)r) atomicMin(&a.first[s], (u32)r);
}

__global__ void __launch_bounds__(256) dict_first_kernel(const CsvDictArgs a) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.f.nrows) return;
    a.rank[r] = ((a.f.lenesc[r] >> 1) > 0 && a.first[a.row_slot[r]] == (u32)r) ? 1 : 0;
}

__global__ void __launch_bounds__(256) dict_codes_kernel(const CsvDictArgs a) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.f.nrows) return;
    if ((a.f.lenesc[r] >> 1) == 0) { a.codes[r] = 0; return; }
    const u32 f = a.first[a.row_slot[r]];
    const i64 code = a.rank[f];
    a.codes[r] = (int)code;
    if (f == (u32)r) {
        a.dist_row[code] = r;
        a.dist_len[code] = field_bytes(a.f, r).count();
    }
}

// ---- 5. the fields of a row list, unescaped and packed ----------------------------------------------------------------
__global__ void __launch_bounds__(256) field_len_kernel(const CsvFields f, const i64 *rows, i64 n, i64 *len) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) len[i] = field_bytes(f, rows[i]).count();
}

// (named for its first user: the dictionary's distinct strings; the patch list goes through it as well)
__global__ void __launch_bounds__(256) dict_pack_kernel(const CsvFields f, const i64 *rows, i64 n, const i64 *off, unsigned char *packed) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Unesc u = field_bytes(f, rows[i]);
    unsigned char c;
    i64 o = off[i];
    while (u.next(c)) packed[o++] = c;
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------------------------------
void launch_csv_quote_count(hipStream_t s, const unsigned char *text, long long ntiles, long long *tile_quotes) {
    hipLaunchKernelGGL(quote_count_kernel, dim3(grid_of(ntiles, 4)), dim3(256), 0, s, text, ntiles, tile_quotes);
}

void launch_csv_records(hipStream_t s, bool write, const unsigned char *text, long long n, long long ntiles, const long long *tile_quotes,
                        long long *tile_rows, long long *rec_start, unsigned int *flags) {
    const dim3 g(grid_of(ntiles, 4));
    if (write) hipLaunchKernelGGL(records_kernel<true>, g, dim3(256), 0, s, text, n, ntiles, tile_quotes, tile_rows, rec_start, flags);
    else hipLaunchKernelGGL(records_kernel<false>, g, dim3(256), 0, s, text, n, ntiles, tile_quotes, tile_rows, rec_start, flags);
}

void launch_csv_spans(hipStream_t s, const CsvSpanArgs &a) {
    hipLaunchKernelGGL(spans_kernel, dim3(grid_of(a.all.nrows, 256)), dim3(256), 0, s, a);
}

void launch_csv_convert_double(hipStream_t s, const CsvConvArgs &a) {
    hipLaunchKernelGGL(convert_double_kernel, dim3(grid_of(a.f.nrows, 256)), dim3(256), 0, s, a);
}

void launch_csv_convert_bool(hipStream_t s, const CsvConvArgs &a) {
    hipLaunchKernelGGL(convert_bool_kernel, dim3(grid_of(a.f.nrows, 256)), dim3(256), 0, s, a);
}

void launch_csv_scatter_f64(hipStream_t s, double *data, const long long *rows, const double *values, long long n) {
    hipLaunchKernelGGL(scatter_f64_kernel, dim3(grid_of(n, 256)), dim3(256), 0, s, data, rows, values, n);
}

void launch_csv_dict_build(hipStream_t s, const CsvDictArgs &a) {
    const dim3 g(grid_of(a.f.nrows, 256));
    hipLaunchKernelGGL(dict_hash_kernel, g, dim3(256), 0, s, a);
    hipLaunchKernelGGL(dict_insert_kernel, g, dim3(256), 0, s, a);
    hipLaunchKernelGGL(dict_first_kernel, g, dim3(256), 0, s, a);
}

void launch_csv_dict_codes(hipStream_t s, const CsvDictArgs &a) {
    hipLaunchKernelGGL(dict_codes_kernel, dim3(grid_of(a.f.nrows, 256)), dim3(256), 0, s, a);
}

void launch_csv_field_len(hipStream_t s, const CsvFields &f, const long long *rows, long long n, long long *len) {
    hipLaunchKernelGGL(field_len_kernel, dim3(grid_of(n, 256)), dim3(256), 0, s, f, rows, n, len);
}

void launch_csv_pack_fields(hipStream_t s, const CsvFields &f, const long long *rows, long long n, const long long *off, unsigned char *packed) {
    hipLaunchKernelGGL(dict_pack_kernel, dim3(grid_of(n, 256)), dim3(256), 0, s, f, rows, n, off, packed);
}

}  // namespace qe
