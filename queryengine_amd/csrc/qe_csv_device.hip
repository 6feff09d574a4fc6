// qe_csv_device.hip -- CSV text -> qe_batch with the parsing on the device.
//
// The host resolves the header (the first non-empty record, through the host parser's next_record) and copies the text after
// it to HBM through pinned staging.  Then, on the device:
//   1. quote counts per 4 KiB tile, exclusive scan: the quote parity at every tile start;
//   2. one wave per tile walks its bytes 64 at a time: a ballot of the quotes gives the parity before every byte, so the
//      line ends outside quotes, and with them the starts of the non-empty records, are known byte-parallel.  The same pass
//      proves that every '"' is the enclosing quote of a field -- an opening quote (even parity) follows the text start,
//      ',', '\n', '\r' or '"', a closing one (odd parity) precedes the text end, ',', '\n', '\r' or '"' -- which is exactly
//      when quote parity equals the sequential state machine of next_record.  A count pass, a scan, then a write pass
//      that stores the record starts in row order;
//   3. one thread per record walks its fields and notes the span of every projected one;
//   4. one thread per row and column converts: DOUBLE through qe_csv_number.h (fields it leaves undecided go to a patch
//      list the host converts), BOOLEAN, validity -- bitmaps as one ballot per 64 rows; STRING fields are hashed, inserted
//      into an open-addressing table (bytes compared on a hash match), numbered by their first row (a scan over the rows
//      that are the first of their string) and the distinct strings packed for the host's dictionary.
// Whatever the device cannot prove it reads as the host does (a quote against the rule above, an unterminated quote, a
// field that is no number) sends the whole input through qe_csv_parse + qe_csv_pin: same result or the same error.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <thread>

#include "qe_exec.h"
#include "qe_csv_number.h"
#include "qe_scan.h"

using i64 = long long;
using u64 = unsigned long long;
using u32 = unsigned int;

namespace {

constexpr int kTile = 4096;          // text bytes per wave in the structure passes (64 steps of 64 bytes)
constexpr u32 kEmpty = 0xFFFFFFFFu;

// what the structure pass found that the host parser would read differently
enum { F_QUOTE_RULE = 1, F_BAD_NUMBER = 2, F_PATCH_OVERFLOW = 4 };

__device__ inline bool is_sep(unsigned char c) { return c == ',' || c == '\n' || c == '\r' || c == '"'; }

// ---- 1. quotes per tile ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) quote_count_kernel(const unsigned char *text, i64 ntiles, i64 *tile_quotes) {
    const i64 tile = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (tile >= ntiles) return;
    // the text buffer is padded with zero bytes to whole tiles: every lane reads its 64 bytes unguarded
    const uint4 *p = (const uint4 *)(text + tile * kTile + lane * 64);
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
    const i64 tile = (i64)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (tile >= ntiles) return;
    const u64 lt = (1ull << lane) - 1;
    const i64 base = tile * kTile;
    u32 parity = (u32)(tile_quotes_before[tile] & 1);
    unsigned char carry_prev = base > 0 ? text[base - 1] : 0;   // the byte in front of this step's lane 0
    i64 out = WRITE ? tile_rows[tile] : 0;
    i64 count = 0;
    bool bad = false;
    for (int s = 0; s < kTile / 64; s++) {
        const i64 i = base + s * 64 + lane;
        const unsigned char c = i < n ? text[i] : 0;
        unsigned char prev = (unsigned char)qe::wave_prev((int)c);
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
        if (__any(bad) && lane == 0) atomicOr(flags, (u32)F_QUOTE_RULE);
        if (lane == 0) tile_rows[tile] = count;
    }
}

// ---- 3. field spans --------------------------------------------------------------------------------------------------
// span of projected column k in row r: begin[k * nrows + r] = first content byte, lenesc[..] = content bytes << 1 | (the
// content holds "" escapes).  Length 0 = NULL (empty, "" or missing).
struct SpanArgs {
    const unsigned char *text;
    i64 n;
    const i64 *rec_start;
    i64 nrows;
    const int *field_of;   // per projected column: field index in the record
    int ncols;
    int max_field;
    i64 *begin;
    u32 *lenesc;
};

__global__ void __launch_bounds__(256) spans_kernel(const SpanArgs a) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.nrows) return;
    for (int k = 0; k < a.ncols; k++) { a.begin[k * a.nrows + r] = 0; a.lenesc[k * a.nrows + r] = 0; }
    const unsigned char *t = a.text;
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
                a.begin[k * a.nrows + r] = cb;
                a.lenesc[k * a.nrows + r] = (u32)(ce - cb) << 1 | esc;
            }
        if (pos >= a.n || t[pos] != ',') break;   // the record ends; later fields are missing
        pos++;
    }
}

// one 64-row word of a bitmap per wave; any_null is raised when a word misses a row that exists
__device__ inline void store_bits(u64 *words, u32 *any_null, i64 r, i64 nrows, bool value, bool valid, u64 *validity) {
    const u64 vb = __ballot(valid);
    const u64 bb = __ballot(value);
    if ((threadIdx.x & 63) == 0 && r < nrows) {
        const i64 left = nrows - r;
        const u64 full = left >= 64 ? ~0ull : ((1ull << left) - 1);
        if (words) words[r >> 6] = bb;
        validity[r >> 6] = vb;
        if (vb != full) atomicOr(any_null, 1u);
    }
}

// ---- 4a. DOUBLE / BOOLEAN --------------------------------------------------------------------------------------------
struct ConvArgs {
    const unsigned char *text;
    i64 nrows;
    const i64 *begin;
    const u32 *lenesc;
    void *data;
    u64 *validity;
    u32 *any_null;
    u32 *flags;
    i64 *patch_rows;    // DOUBLE: rows the host converts
    u32 *patch_count;
    u32 patch_cap;
};

__global__ void __launch_bounds__(256) convert_double_kernel(const ConvArgs a) {
    const i64 r0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63);
    const i64 r = r0 + (threadIdx.x & 63);
    bool valid = false;
    if (r < a.nrows) {
        const u32 le = a.lenesc[r];
        const u32 len = le >> 1;
        double v = 0.0;
        if (len > 0) {
            valid = true;
            if (le & 1) {
                atomicOr(a.flags, (u32)F_BAD_NUMBER);   // a '"' inside: no Java literal
            } else {
                const int st = qe_parse_double(a.text + a.begin[r], len, v);
                if (st == QE_NUM_REJECT) {
                    atomicOr(a.flags, (u32)F_BAD_NUMBER);
                } else if (st == QE_NUM_UNDECIDED) {
                    const u32 slot = atomicAdd(a.patch_count, 1u);
                    if (slot < a.patch_cap) a.patch_rows[slot] = r;
                    else atomicOr(a.flags, (u32)F_PATCH_OVERFLOW);
                    v = 0.0;
                }
            }
        }
        ((double *)a.data)[r] = v;
    }
    store_bits(nullptr, a.any_null, r0, a.nrows, false, valid, a.validity);
}

__global__ void __launch_bounds__(256) convert_bool_kernel(const ConvArgs a) {
    const i64 r0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63);
    const i64 r = r0 + (threadIdx.x & 63);
    bool valid = false, value = false;
    if (r < a.nrows) {
        const u32 le = a.lenesc[r];
        valid = (le >> 1) > 0;
        if (le == (4u << 1)) {   // exactly four bytes, no escape: String.toBoolean
            const unsigned char *p = a.text + a.begin[r];
            value = (p[0] | 0x20) == 't' && (p[1] | 0x20) == 'r' && (p[2] | 0x20) == 'u' && (p[3] | 0x20) == 'e';
        }
    }
    store_bits((u64 *)a.data, a.any_null, r0, a.nrows, value, valid, a.validity);
}

__global__ void __launch_bounds__(256) scatter_f64_kernel(double *data, const i64 *rows, const double *values, i64 n) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n) data[rows[i]] = values[i];
}

// ---- 4b. STRING: device dictionary ------------------------------------------------------------------------------------
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
};

__device__ inline u64 mix64(u64 h) {
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull;
    return h ^ (h >> 33);
}

struct DictArgs {
    const unsigned char *text;
    i64 nrows;
    const i64 *begin;
    const u32 *lenesc;
    u64 *hash;          // per row: FNV-1a of the unescaped bytes
    u32 *slots;         // open-addressing table: the row that represents the entry's string
    u32 *first;         // .. the smallest row holding it
    u64 mask;
    u32 *row_slot;      // per row: its entry
    i64 *rank;          // per row: 1 if the row is the first of its string, then (scanned) the code it gives that string
    int *codes;
    i64 *dist_row;      // per code: the first row
    i64 *dist_len;      // per code: unescaped bytes, then (scanned) the offset in `packed`
    unsigned char *packed;
    u64 *validity;
    u32 *any_null;
};

__global__ void __launch_bounds__(256) dict_hash_kernel(const DictArgs a) {
    const i64 r0 = (i64)blockIdx.x * 256 + (threadIdx.x & ~63);
    const i64 r = r0 + (threadIdx.x & 63);
    bool valid = false;
    if (r < a.nrows) {
        const u32 le = a.lenesc[r];
        valid = (le >> 1) > 0;
        u64 h = 0xcbf29ce484222325ull;
        Unesc u{a.text, a.begin[r], a.begin[r] + (le >> 1), (le & 1) != 0};
        unsigned char c;
        while (u.next(c)) h = (h ^ c) * 0x100000001b3ull;
        a.hash[r] = h;
    }
    store_bits(nullptr, a.any_null, r0, a.nrows, false, valid, a.validity);
}

__device__ inline bool same_string(const DictArgs &a, i64 x, i64 y) {
    const u32 lx = a.lenesc[x], ly = a.lenesc[y];
    Unesc ux{a.text, a.begin[x], a.begin[x] + (lx >> 1), (lx & 1) != 0};
    Unesc uy{a.text, a.begin[y], a.begin[y] + (ly >> 1), (ly & 1) != 0};
    if (!ux.esc && !uy.esc && lx != ly) return false;
    for (;;) {
        unsigned char cx, cy;
        const bool hx = ux.next(cx), hy = uy.next(cy);
        if (hx != hy) return false;
        if (!hx) return true;
        if (cx != cy) return false;
    }
}

__global__ void __launch_bounds__(256) dict_insert_kernel(const DictArgs a) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.nrows || (a.lenesc[r] >> 1) == 0) return;
    const u64 h = a.hash[r];
    u64 s = mix64(h) & a.mask;
    for (;;) {
        u32 cur = __hip_atomic_load(&a.slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty) {
            const u32 prev = atomicCAS(&a.slots[s], kEmpty, (u32)r);
            cur = prev == kEmpty ? (u32)r : prev;
        }
        if (cur == (u32)r || (a.hash[cur] == h && same_string(a, r, cur))) break;
        s = (s + 1) & a.mask;
    }
    a.row_slot[r] = (u32)s;
    // rows arrive roughly in order: most see a first row at or below their own and skip the atomic
    if (__hip_atomic_load(&a.first[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (u32)r) atomicMin(&a.first[s], (u32)r);
}

__global__ void __launch_bounds__(256) dict_first_kernel(const DictArgs a) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.nrows) return;
    a.rank[r] = ((a.lenesc[r] >> 1) > 0 && a.first[a.row_slot[r]] == (u32)r) ? 1 : 0;
}

__global__ void __launch_bounds__(256) dict_codes_kernel(const DictArgs a) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.nrows) return;
    const u32 le = a.lenesc[r];
    if ((le >> 1) == 0) { a.codes[r] = 0; return; }
    const u32 f = a.first[a.row_slot[r]];
    const i64 code = a.rank[f];
    a.codes[r] = (int)code;
    if (f == (u32)r) {
        a.dist_row[code] = r;
        i64 len = 0;
        Unesc u{a.text, a.begin[r], a.begin[r] + (le >> 1), (le & 1) != 0};
        unsigned char c;
        while (u.next(c)) len++;
        a.dist_len[code] = len;
    }
}

__global__ void __launch_bounds__(256) dict_pack_kernel(const DictArgs a, i64 ndistinct) {
    const i64 d = (i64)blockIdx.x * 256 + threadIdx.x;
    if (d >= ndistinct) return;
    const i64 r = a.dist_row[d];
    const u32 le = a.lenesc[r];
    Unesc u{a.text, a.begin[r], a.begin[r] + (le >> 1), (le & 1) != 0};
    unsigned char c;
    i64 o = a.dist_len[d];
    while (u.next(c)) a.packed[o++] = c;
}

inline unsigned grid_of(i64 n, i64 per) { return (unsigned)std::max<i64>(1, (n + per - 1) / per); }

}  // namespace

// ---- host side ----------------------------------------------------------------------------------------------------------
using namespace qe;

namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// n elements of T among the device buffers of one call (PoolScratch returns them to the context's pool on every exit)
template <typename T>
T *dev_array(PoolScratch &S, size_t n) { return (T *)S.alloc(n * sizeof(T)); }

// exclusive sum of a[0..n) in place; a must hold n + 1 elements, a[n] = 0 on entry: the total lands in a[n]
void scan(qe_ctx *ctx, PoolScratch &S, i64 *a, i64 n) {
    exclusive_scan<i64>(ctx->stream, ArrayLoad<i64>{a}, a, dev_array<i64>(S, (size_t)scan_blocks(n + 1)), n + 1, nullptr);
}

template <typename T>
T read_back(qe_ctx *ctx, const T *dev) {
    T v{};
    QE_HIP(hipMemcpyAsync(&v, dev, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    return v;
}

struct FallBack {};   // the device cannot prove its reading equal to the host parser's: the host parses the input

struct Request {
    int32_t nfields;
    const char *const *names;
    const int32_t *types;
};

// The header: the first non-empty record, names resolved to their LAST occurrence.  Returns false where the host parser
// would fail (no header, a missing name, a malformed quoted field, a bad type) -- its error text is the host's.
bool resolve_header(const char *data, size_t n, const Request &rq, size_t &body, std::vector<int> &idx) {
    for (int32_t k = 0; k < rq.nfields; k++) {
        if (!rq.names[k]) return false;
        if (rq.types[k] != QE_STRING && rq.types[k] != QE_DOUBLE && rq.types[k] != QE_BOOLEAN) return false;
    }
    std::vector<Field> rec;
    std::string unq;
    std::vector<std::pair<size_t, size_t>> span;
    size_t pos = 0;
    bool empty = false;
    idx.assign((size_t)rq.nfields, -1);
    try {
        while (next_record(data, n, pos, rec, unq, span, empty)) {
            if (empty) continue;
            for (int32_t k = 0; k < rq.nfields; k++)
                for (size_t i = 0; i < rec.size(); i++) {
                    const Field &f = rec[i];
                    const char *p = f.quoted ? unq.data() + span[f.begin].first : data + f.begin;
                    const size_t m = f.quoted ? span[f.begin].second - span[f.begin].first : f.end - f.begin;
                    if (m == std::strlen(rq.names[k]) && std::memcmp(p, rq.names[k], m) == 0) idx[(size_t)k] = (int)i;
                }
            break;
        }
    } catch (const Error &) {
        return false;
    }
    for (int v : idx)
        if (v < 0) return false;
    body = pos;
    return true;
}

// Source of the text after the header: bytes [off, off + n) into a pinned chunk, callable from several threads.
struct TextSource {
    virtual ~TextSource() {}
    virtual void read_at(char *dst, size_t off, size_t n) = 0;   // exactly n bytes or throws
};

// Fill a chunk with a few host threads: one memcpy / pread thread moves ~10 GB/s, the link ~55 GB/s.
void parallel_read(TextSource &src, char *dst, size_t off, size_t n) {
    const size_t kMin = 4u << 20;
    const unsigned nthr = (unsigned)std::min<size_t>(8, std::max<size_t>(1, n / kMin));
    if (nthr <= 1) {
        src.read_at(dst, off, n);
        return;
    }
    // whole pages per thread, rounded UP twice: n / nthr rounded down leaves the last n % nthr bytes to nobody when it is a
    // whole number of pages already
    const size_t per = (((n + nthr - 1) / nthr) + 4095) & ~(size_t)4095;
    std::vector<std::thread> ts;
    std::vector<std::string> errs(nthr);
    for (unsigned t = 1; t < nthr; t++) {
        const size_t o = (size_t)t * per;
        if (o >= n) break;
        const size_t len = std::min(per, n - o);
        ts.emplace_back([&, t, o, len] {
            try { src.read_at(dst + o, off + o, len); } catch (const Error &e) { errs[t] = e.msg.empty() ? "read error" : e.msg; }
        });
    }
    try { src.read_at(dst, off, std::min(per, n)); } catch (const Error &e) { errs[0] = e.msg.empty() ? "read error" : e.msg; }
    for (auto &t : ts) t.join();
    for (auto &e : errs)
        if (!e.empty()) fail(QE_ERR_INVALID_ARG, e);
}

// text -> HBM through two pinned chunks: the fill of one runs beside the copy of the other
void upload(qe_ctx *ctx, TextSource &src, unsigned char *dev, size_t n) {
    if (n == 0) return;
    const size_t chunk = (size_t)64 << 20;
    char *pin[2] = {(char *)ctx->pinned.alloc(std::min(chunk, n)), nullptr};
    struct Rel { qe_ctx *c; char **p; ~Rel() { c->pinned.release(p[0]); c->pinned.release(p[1]); } } rel{ctx, pin};
    if (n > chunk) pin[1] = (char *)ctx->pinned.alloc(chunk);
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvRel { hipEvent_t *e; ~EvRel() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evrel{ev};
    QE_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
    QE_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
    bool used[2] = {false, false};
    for (size_t off = 0, k = 0; off < n; off += chunk, k++) {
        const int b = (int)(k & 1);
        const size_t m = std::min(chunk, n - off);
        if (used[b]) QE_HIP(hipEventSynchronize(ev[b]));   // the copy out of this chunk two steps ago has finished
        parallel_read(src, pin[b], off, m);
        QE_HIP(hipMemcpyAsync(dev + off, pin[b], m, hipMemcpyHostToDevice, ctx->stream));
        QE_HIP(hipEventRecord(ev[b], ctx->stream));
        used[b] = true;
    }
    QE_HIP(hipStreamSynchronize(ctx->stream));
}

struct MemSource : TextSource {
    const char *p;
    explicit MemSource(const char *q) : p(q) {}
    void read_at(char *dst, size_t off, size_t n) override { std::memcpy(dst, p + off, n); }
};

struct FileSource : TextSource {
    int fd;
    size_t base;
    std::string path;
    FileSource(int f, size_t b, std::string s) : fd(f), base(b), path(std::move(s)) {}
    void read_at(char *dst, size_t off, size_t n) override {
        while (n > 0) {
            const ssize_t r = ::pread(fd, dst, n, (off_t)(base + off));
            if (r <= 0) {
                if (r < 0 && errno == EINTR) continue;
                fail(QE_ERR_INVALID_ARG, "read error on " + path);
            }
            dst += r; off += (size_t)r; n -= (size_t)r;
        }
    }
};

struct BatchDeleter {
    qe_ctx *ctx;
    void operator()(qe_batch *b) const { free_batch(ctx, b); }
};

// The device passes over the text in `dev` (n bytes, padded with zeros to whole tiles).  Throws FallBack.
qe_batch *parse_on_device(qe_ctx *ctx, PoolScratch &S, const unsigned char *dev, i64 n, const Request &rq, const std::vector<int> &idx) {
    hipStream_t st = ctx->stream;
    const i64 ntiles = (n + kTile - 1) / kTile;
    u32 *flags = dev_array<u32>(S, 4);
    QE_HIP(hipMemsetAsync(flags, 0, 16, st));
    i64 nrows = 0;
    i64 *rec_start = nullptr;
    if (ntiles > 0) {
        i64 *tq = dev_array<i64>(S, (size_t)ntiles + 1);
        QE_HIP(hipMemsetAsync(tq + ntiles, 0, sizeof(i64), st));
        hipLaunchKernelGGL(quote_count_kernel, dim3(grid_of(ntiles, 4)), dim3(256), 0, st, dev, ntiles, tq);
        scan(ctx, S, tq, ntiles);
        if (read_back(ctx, tq + ntiles) & 1) throw FallBack{};   // an unterminated quote
        i64 *tr = dev_array<i64>(S, (size_t)ntiles + 1);
        QE_HIP(hipMemsetAsync(tr + ntiles, 0, sizeof(i64), st));
        hipLaunchKernelGGL(records_kernel<false>, dim3(grid_of(ntiles, 4)), dim3(256), 0, st, dev, n, ntiles, (const i64 *)tq, tr,
                           (i64 *)nullptr, flags);
        scan(ctx, S, tr, ntiles);
        nrows = read_back(ctx, tr + ntiles);
        if (read_back(ctx, flags) & F_QUOTE_RULE) throw FallBack{};
        if (nrows >= (i64)0x7FFFFFFF) throw FallBack{};   // row ids of the dictionary table are 32-bit
        rec_start = dev_array<i64>(S, (size_t)nrows + 1);
        hipLaunchKernelGGL(records_kernel<true>, dim3(grid_of(ntiles, 4)), dim3(256), 0, st, dev, n, ntiles, (const i64 *)tq, tr,
                           rec_start, flags);
    }
    const int ncols = rq.nfields;
    i64 *begin = nullptr;
    u32 *lenesc = nullptr;
    if (nrows > 0 && ncols > 0) {
        begin = dev_array<i64>(S, (size_t)ncols * nrows);
        lenesc = dev_array<u32>(S, (size_t)ncols * nrows);
        int *field_of = dev_array<int>(S, (size_t)ncols);
        QE_HIP(hipMemcpyAsync(field_of, idx.data(), sizeof(int) * ncols, hipMemcpyHostToDevice, st));
        SpanArgs a{dev, n, rec_start, nrows, field_of, ncols, *std::max_element(idx.begin(), idx.end()), begin, lenesc};
        hipLaunchKernelGGL(spans_kernel, dim3(grid_of(nrows, 256)), dim3(256), 0, st, a);
    }
    // the batch: column buffers sized like qe_batch_create's
    std::unique_ptr<qe_batch, BatchDeleter> b(new qe_batch(), BatchDeleter{ctx});   // its columns go back to the pool unless it is released
    b->nrows = nrows;
    const size_t words = (size_t)((nrows + 63) / 64);
    u32 *any_null = dev_array<u32>(S, (size_t)std::max(ncols, 1));
    QE_HIP(hipMemsetAsync(any_null, 0, sizeof(u32) * std::max(ncols, 1), st));
    u32 *patch_count = dev_array<u32>(S, 1);
    const u32 patch_cap = (u32)std::min<i64>(std::max<i64>(nrows, 1), 1 << 20);
    i64 *patch_rows = dev_array<i64>(S, patch_cap);
    std::vector<int> dict_cols;
    for (int k = 0; k < ncols; k++) {
        Column c;
        c.type = rq.types[k];
        const size_t nb = c.type == QE_BOOLEAN ? words * 8 : (size_t)nrows * (c.type == QE_DOUBLE ? 8 : 4);
        c.data = ctx->pool.alloc(nb);
        if (nrows > 0) c.validity = (uint64_t *)ctx->pool.alloc(words * 8);
        if (c.type == QE_STRING) c.dict = std::make_shared<DictData>();
        b->cols.push_back(c);
        if (nrows == 0) continue;
        const i64 *kb = begin + (size_t)k * nrows;
        const u32 *kl = lenesc + (size_t)k * nrows;
        if (c.type == QE_DOUBLE || c.type == QE_BOOLEAN) {
            QE_HIP(hipMemsetAsync(patch_count, 0, sizeof(u32), st));
            ConvArgs a{dev, nrows, kb, kl, c.data, (u64 *)c.validity, any_null + k, flags, patch_rows, patch_count, patch_cap};
            if (c.type == QE_DOUBLE) {
                hipLaunchKernelGGL(convert_double_kernel, dim3(grid_of(nrows, 256)), dim3(256), 0, st, a);
                const u32 np = read_back(ctx, patch_count);
                const u32 fl = read_back(ctx, flags);
                if (fl & (F_BAD_NUMBER | F_PATCH_OVERFLOW)) throw FallBack{};
                if (np > 0) {   // the fields the device left undecided: the host's converter, then one scatter
                    std::vector<i64> rows(np), fb(np);
                    std::vector<u32> fl2(np);
                    QE_HIP(hipMemcpyAsync(rows.data(), patch_rows, sizeof(i64) * np, hipMemcpyDeviceToHost, st));
                    QE_HIP(hipStreamSynchronize(st));
                    std::vector<double> vals(np);
                    std::string txt;
                    for (u32 j = 0; j < np; j++) {
                        QE_HIP(hipMemcpyAsync(&fb[j], kb + rows[j], sizeof(i64), hipMemcpyDeviceToHost, st));
                        QE_HIP(hipMemcpyAsync(&fl2[j], kl + rows[j], sizeof(u32), hipMemcpyDeviceToHost, st));
                    }
                    QE_HIP(hipStreamSynchronize(st));
                    for (u32 j = 0; j < np; j++) {
                        txt.resize(fl2[j] >> 1);
                        QE_HIP(hipMemcpy(&txt[0], dev + fb[j], txt.size(), hipMemcpyDeviceToHost));
                        if (!java_parse_double(txt.data(), txt.size(), vals[j])) throw FallBack{};
                    }
                    i64 *drows = dev_array<i64>(S, np);
                    double *dvals = dev_array<double>(S, np);
                    QE_HIP(hipMemcpyAsync(drows, rows.data(), sizeof(i64) * np, hipMemcpyHostToDevice, st));
                    QE_HIP(hipMemcpyAsync(dvals, vals.data(), sizeof(double) * np, hipMemcpyHostToDevice, st));
                    hipLaunchKernelGGL(scatter_f64_kernel, dim3(grid_of(np, 256)), dim3(256), 0, st, (double *)c.data,
                                       (const i64 *)drows, (const double *)dvals, (i64)np);
                    QE_HIP(hipStreamSynchronize(st));
                    ctx->csv_stats.host_patched_fields += np;
                }
            } else {
                hipLaunchKernelGGL(convert_bool_kernel, dim3(grid_of(nrows, 256)), dim3(256), 0, st, a);
            }
            continue;
        }
        // STRING
        dict_cols.push_back(k);
        u64 cap = 64;
        while (cap < (u64)nrows * 2) cap <<= 1;
        DictArgs a{};
        a.text = dev;
        a.nrows = nrows;
        a.begin = kb;
        a.lenesc = kl;
        a.hash = dev_array<u64>(S, (size_t)nrows);
        a.slots = dev_array<u32>(S, cap);
        a.first = dev_array<u32>(S, cap);
        a.mask = cap - 1;
        a.row_slot = dev_array<u32>(S, (size_t)nrows);
        a.rank = dev_array<i64>(S, (size_t)nrows + 1);
        a.codes = (int *)c.data;
        a.validity = (u64 *)c.validity;
        a.any_null = any_null + k;
        QE_HIP(hipMemsetAsync(a.slots, 0xFF, cap * sizeof(u32), st));
        QE_HIP(hipMemsetAsync(a.first, 0xFF, cap * sizeof(u32), st));
        QE_HIP(hipMemsetAsync(a.rank + nrows, 0, sizeof(i64), st));
        const dim3 g(grid_of(nrows, 256));
        hipLaunchKernelGGL(dict_hash_kernel, g, dim3(256), 0, st, a);
        hipLaunchKernelGGL(dict_insert_kernel, g, dim3(256), 0, st, a);
        hipLaunchKernelGGL(dict_first_kernel, g, dim3(256), 0, st, a);
        scan(ctx, S, a.rank, nrows);
        const i64 nd = read_back(ctx, a.rank + nrows);
        a.dist_row = dev_array<i64>(S, (size_t)nd);
        a.dist_len = dev_array<i64>(S, (size_t)nd + 1);
        QE_HIP(hipMemsetAsync(a.dist_len + nd, 0, sizeof(i64), st));
        hipLaunchKernelGGL(dict_codes_kernel, g, dim3(256), 0, st, a);
        scan(ctx, S, a.dist_len, nd);
        std::vector<i64> off((size_t)nd + 1);
        QE_HIP(hipMemcpyAsync(off.data(), a.dist_len, sizeof(i64) * (nd + 1), hipMemcpyDeviceToHost, st));
        QE_HIP(hipStreamSynchronize(st));
        a.packed = dev_array<unsigned char>(S, (size_t)off[(size_t)nd]);
        hipLaunchKernelGGL(dict_pack_kernel, dim3(grid_of(nd, 256)), dim3(256), 0, st, a, nd);
        std::string bytes((size_t)off[(size_t)nd], '\0');
        if (!bytes.empty())
            QE_HIP(hipMemcpyAsync(&bytes[0], a.packed, bytes.size(), hipMemcpyDeviceToHost, st));
        QE_HIP(hipStreamSynchronize(st));
        DictData &d = *b->cols.back().dict;
        d.entries.reserve((size_t)nd);
        for (i64 j = 0; j < nd; j++) {
            d.entries.emplace_back(bytes, (size_t)off[(size_t)j], (size_t)(off[(size_t)j + 1] - off[(size_t)j]));
            d.index.emplace(d.entries.back(), (int32_t)j);
        }
    }
    QE_HIP(hipGetLastError());
    if (nrows > 0) {
        std::vector<u32> nulls((size_t)ncols);
        if (ncols > 0)
            QE_HIP(hipMemcpyAsync(nulls.data(), any_null, sizeof(u32) * ncols, hipMemcpyDeviceToHost, st));
        QE_HIP(hipStreamSynchronize(st));
        for (int k = 0; k < ncols; k++)
            if (!nulls[(size_t)k]) {   // no NULL: no validity bitmap, like the host's any_null
                ctx->pool.release(b->cols[(size_t)k].validity);
                b->cols[(size_t)k].validity = nullptr;
            }
    }
    QE_HIP(hipStreamSynchronize(st));
    return b.release();
}

template <typename F>
int32_t guarded_dev(qe_ctx *ctx, F &&f) {
    try {
        f();
        return QE_OK;
    } catch (const Error &e) {
        ctx->last_error = e.msg;
        return e.code;
    } catch (const std::bad_alloc &) {
        ctx->last_error = "host out of memory";
        return QE_ERR_OOM;
    } catch (const std::exception &e) {
        ctx->last_error = e.what();
        return QE_ERR_INTERNAL;
    }
}

int32_t check_args(qe_ctx *ctx, int32_t nfields, const char *const *names, const int32_t *types, qe_batch **out) {
    if (!ctx || !out || nfields < 0 || (nfields > 0 && (!names || !types))) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    ctx->csv_stats = qe_csv_device_stats{};
    if (ctx->device < 0) {
        ctx->last_error = "planning-only context (QE_DEVICE_NONE): qe_csv_parse_device needs a HIP device; libqe_hip has no CPU fallback";
        return QE_ERR_HIP;
    }
    return QE_OK;
}

unsigned char *alloc_text(qe_ctx *ctx, PoolScratch &S, size_t n) {
    const size_t padded = ((n + kTile - 1) / kTile) * kTile + 64;
    void *p = nullptr;
    try {
        p = dev_array<unsigned char>(S, padded);
    } catch (const Error &e) {
        fail(QE_ERR_OOM, "CSV text of " + std::to_string(n) + " bytes does not fit in free device memory (" + e.msg + ")");
    }
    QE_HIP(hipMemsetAsync((char *)p + n, 0, padded - n, ctx->stream));   // the passes read whole tiles
    return (unsigned char *)p;
}

}  // namespace

extern "C" {

int32_t qe_csv_parse_device(qe_ctx *ctx, const char *data, size_t nbytes, int32_t nfields, const char *const *names,
                            const int32_t *types, qe_batch **out) {
    int32_t st = check_args(ctx, nfields, names, types, out);
    if (st != QE_OK) return st;
    if (!data && nbytes) return QE_ERR_INVALID_ARG;
    ctx->csv_stats.text_bytes = (int64_t)nbytes;
    bool fallback = false;
    st = guarded_dev(ctx, [&] {
        QE_HIP(hipSetDevice(ctx->device));
        const Request rq{nfields, names, types};
        size_t body = 0;
        std::vector<int> idx;
        if (!resolve_header(data, nbytes, rq, body, idx)) { fallback = true; return; }
        PoolScratch S(ctx);
        const size_t n = nbytes - body;
        auto t0 = Clock::now();
        unsigned char *dev = alloc_text(ctx, S, n);
        MemSource src(data + body);
        upload(ctx, src, dev, n);
        ctx->csv_stats.h2d_ms = ms_since(t0);
        t0 = Clock::now();
        try {
            *out = parse_on_device(ctx, S, dev, (i64)n, rq, idx);
        } catch (const FallBack &) {
            fallback = true;
            ctx->csv_stats.host_patched_fields = 0;
            return;
        }
        ctx->csv_stats.kernel_ms = ms_since(t0);
        ctx->csv_stats.nrows = (*out)->nrows;
    });
    if (st != QE_OK || !fallback) return st;
    ctx->csv_stats.host_fallback = 1;
    qe_csv_table *t = nullptr;
    st = qe_csv_parse(ctx, data, nbytes, nfields, names, types, &t);
    if (st != QE_OK) return st;
    st = qe_csv_pin(ctx, t, out);
    if (st == QE_OK) ctx->csv_stats.nrows = qe_csv_nrows(t);
    qe_csv_free(ctx, t);
    return st;
}

int32_t qe_csv_parse_file_device(qe_ctx *ctx, const char *path, int32_t nfields, const char *const *names,
                                 const int32_t *types, qe_batch **out) {
    int32_t st = check_args(ctx, nfields, names, types, out);
    if (st != QE_OK) return st;
    if (!path) return QE_ERR_INVALID_ARG;
    bool fallback = false;
    st = guarded_dev(ctx, [&] {
        QE_HIP(hipSetDevice(ctx->device));
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) fail(QE_ERR_INVALID_ARG, std::string("cannot open ") + path + ": " + std::strerror(errno));
        struct Closer { int fd; ~Closer() { ::close(fd); } } closer{fd};
        struct stat sb;
        if (::fstat(fd, &sb) != 0) fail(QE_ERR_INVALID_ARG, std::string("read error on ") + path);
        const size_t nbytes = (size_t)sb.st_size;
        ctx->csv_stats.text_bytes = (int64_t)nbytes;
        // the header from the first 1 MiB; a header that does not end there goes the host's way
        std::vector<char> head(std::min<size_t>(nbytes, (size_t)1 << 20));
        if (!head.empty()) FileSource(fd, 0, path).read_at(head.data(), 0, head.size());
        const Request rq{nfields, names, types};
        size_t body = 0;
        std::vector<int> idx;
        if (!resolve_header(head.data(), head.size(), rq, body, idx) || (body == head.size() && head.size() < nbytes)) {
            fallback = true;
            return;
        }
        PoolScratch S(ctx);
        const size_t n = nbytes - body;
        auto t0 = Clock::now();
        unsigned char *dev = alloc_text(ctx, S, n);
        FileSource src(fd, body, path);
        upload(ctx, src, dev, n);
        ctx->csv_stats.h2d_ms = ms_since(t0);
        t0 = Clock::now();
        try {
            *out = parse_on_device(ctx, S, dev, (i64)n, rq, idx);
        } catch (const FallBack &) {
            fallback = true;
            ctx->csv_stats.host_patched_fields = 0;
            return;
        }
        ctx->csv_stats.kernel_ms = ms_since(t0);
        ctx->csv_stats.nrows = (*out)->nrows;
    });
    if (st != QE_OK || !fallback) return st;
    ctx->csv_stats.host_fallback = 1;
    qe_csv_table *t = nullptr;
    st = qe_csv_parse_file(ctx, path, nfields, names, types, &t);
    if (st != QE_OK) return st;
    st = qe_csv_pin(ctx, t, out);
    if (st == QE_OK) ctx->csv_stats.nrows = qe_csv_nrows(t);
    qe_csv_free(ctx, t);
    return st;
}

int32_t qe_csv_device_last_stats(const qe_ctx *ctx, qe_csv_device_stats *out) {
    if (!ctx || !out) return QE_ERR_INVALID_ARG;
    *out = ctx->csv_stats;
    return QE_OK;
}

int32_t qe_batch_column_nullable(const qe_batch *b, int32_t col) {
    if (!b || col < 0 || col >= (int32_t)b->cols.size()) return -1;
    return b->cols[(size_t)col].validity ? 1 : 0;
}

int32_t qe_batch_column_dict(const qe_batch *b, int32_t col, qe_dict **out) {
    if (!b || !out || col < 0 || col >= (int32_t)b->cols.size() || !b->cols[(size_t)col].dict) return QE_ERR_INVALID_ARG;
    *out = new qe_dict{b->cols[(size_t)col].dict};
    return QE_OK;
}

}  // extern "C"
