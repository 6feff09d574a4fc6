// qe_sort.hip -- ORDER BY on the device ("last"): OrderByOperator.open (operator/OrderByOperator.kt:9-15)
// materialises its source and sorts the rows STABLY by one column with Kotlin's compareValues: null first, then
// Double.compareTo (-0.0 < 0.0, NaN greatest) / String.compareTo (UTF-16 code units) / Boolean.compareTo (false < true).
//
// Here the source's result already sits in HBM: (1) the key column becomes one u64 per row whose UNSIGNED order is that
// order (0 = null), (2) the (key, row id) pairs go through a stable LSD radix sort, 4 bits per pass, passes whose digit
// is the same for every key skipped, (3) every column of the result is gathered through the sorted row ids (qe_kernels.hip).  A
// different roofline from the scan (16 read-write passes over 12-byte pairs in the worst case), and not part of any
// BASELINE configuration.
#include <hip/hip_runtime.h>

#include "qe_kernels.h"
#include "qe_scan.h"
#include "qe_sort_image.h"

namespace qe {

// ---- sort keys -----------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) sort_key_kernel(const SortKeyArgs a) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x; j < a.n; j += stride) {
        const i64 i = a.perm ? (i64)a.perm[j] : j;   // a later key of a multi-key sort: the image of the row that stands at j now
        const u64 k = sort_image(a.type, a.data, a.validity, a.ranks, a.nranks, i);   // 0 under a NULL, which the pass on the validity bit (shift 64) moves in front
        // descending: the complement reverses the unsigned order (NULL becomes the greatest image; the validity pass with
        // shift 65 puts it behind every value, also behind a value whose image is all ones)
        a.keys[j] = a.descending ? ~k : k;
        if (!a.perm && a.rows) a.rows[j] = (u32)j;
    }
}
void launch_sort_keys(hipStream_t s, const SortKeyArgs &a) {
    if (a.n <= 0) return;
    const i64 blocks = (a.n + 255) / 256;
    hipLaunchKernelGGL(sort_key_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, a);
}

// OR and AND of all keys: a 4-bit digit whose bits are all equal in both is the same for every key -> its pass is skipped
__global__ void __launch_bounds__(256) key_bits_kernel(const u64 *keys, i64 n, u64 *or_and) {
    u64 o = 0, a = ~0ull;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { o |= keys[i]; a &= keys[i]; }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { o |= __shfl_xor(o, d, 64); a &= __shfl_xor(a, d, 64); }
    if ((threadIdx.x & 63) == 0) { atomicOr(or_and, o); atomicAnd(or_and + 1, a); }
}
void launch_key_bits(hipStream_t s, const unsigned long long *keys, int64_t n, unsigned long long *or_and) {
    if (n <= 0) return;
    const i64 blocks = (n + 255) / 256;
    hipLaunchKernelGGL(key_bits_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, (const u64 *)keys, (i64)n, (u64 *)or_and);
}

// ---- one stable radix pass (4 bits): histogram per block of 1024 elements -> scan -> stable scatter ----------------------
constexpr int kSortBlock = 1024;

// digit of element i: 4 key bits at `shift`, or the validity bit of its row: (shift == 64) NULL (0) before everything else,
// (shift == 65, a descending key) NULL (1) behind everything else
__device__ __forceinline__ int sort_digit(const u64 *keys, const u32 *rows, const u64 *validity, i64 i, int shift) {
    if (shift < 64) return (int)((keys[i] >> shift) & 15ull);
    return (bit_at(validity, (i64)rows[i]) ? 1 : 0) ^ (shift & 1);
}

__global__ void __launch_bounds__(256) radix_hist_kernel(const u64 *keys, const u32 *rows, const u64 *validity, i64 n, int shift, u32 *hist, i64 nblocks) {
    __shared__ u32 s_cnt[16];
    if (threadIdx.x < 16) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const i64 base = (i64)blockIdx.x * kSortBlock;
    for (int r = 0; r < 4; ++r) {
        const i64 i = base + r * 256 + threadIdx.x;
        if (i < n) atomicAdd(&s_cnt[sort_digit(keys, rows, validity, i, shift)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 16) hist[(i64)threadIdx.x * nblocks + blockIdx.x] = s_cnt[threadIdx.x];   // bucket-major: one scan gives the offsets
}

// stable scatter: the block's 1024 elements in 4 rounds of 256 (index order); rank of an element = elements of its digit in
// earlier rounds + in earlier waves of its round + in lower lanes of its wave (__ballot per digit, mbcnt)
__global__ void __launch_bounds__(256) radix_scatter_kernel(const u64 *keys, const u32 *rows, const u64 *validity, i64 n, int shift, const u32 *offsets,
                                                            i64 nblocks, u64 *keys_out, u32 *rows_out) {
    __shared__ u32 s_wave_cnt[4][16];
    __shared__ u32 s_running[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x < 16) s_running[threadIdx.x] = offsets[(i64)threadIdx.x * nblocks + blockIdx.x];
    __syncthreads();
    const i64 base = (i64)blockIdx.x * kSortBlock;
    for (int r = 0; r < 4; ++r) {
        const i64 i = base + r * 256 + threadIdx.x;
        const bool in = i < n;
        const u64 k = in ? keys[i] : 0ull;
        const u32 row = in ? rows[i] : 0u;
        const int digit = in ? sort_digit(keys, rows, validity, i, shift) : 16;
        u32 my_rank = 0;
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            const u64 m = __ballot(digit == d);
            if (digit == d) my_rank = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
            if (lane == 0) s_wave_cnt[wave][d] = (u32)__popcll(m);
        }
        __syncthreads();
        if (in) {
            u32 pos = s_running[digit] + my_rank;
            for (int w = 0; w < wave; ++w) pos += s_wave_cnt[w][digit];
            keys_out[pos] = k;
            rows_out[pos] = row;
        }
        __syncthreads();
        if (threadIdx.x < 16) s_running[threadIdx.x] += s_wave_cnt[0][threadIdx.x] + s_wave_cnt[1][threadIdx.x] + s_wave_cnt[2][threadIdx.x] + s_wave_cnt[3][threadIdx.x];
        __syncthreads();
    }
}

void launch_radix_pass(hipStream_t s, const unsigned long long *keys, const uint32_t *rows, const uint64_t *validity, int64_t n, int shift,
                       uint32_t *hist, unsigned long long *keys_out, uint32_t *rows_out) {
    if (n <= 0) return;
    const i64 nblocks = (n + kSortBlock - 1) / kSortBlock;
    hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, (const u64 *)keys, rows, (const u64 *)validity, (i64)n, shift, hist, nblocks);
    launch_carry_scan<u32, 1024>(s, hist, 16 * nblocks, 1, nullptr);   // the table is small: 16 counters per 1024 rows
    hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, (const u64 *)keys, rows, (const u64 *)validity, (i64)n, shift,
                       (const u32 *)hist, nblocks, (u64 *)keys_out, rows_out);
}

// ---- ORDER BY .. LIMIT k: radix SELECT of the k-th smallest first-key image, then the candidates in row order -----------------
// The images of the first key are only READ here (8 bytes per row and pass, nothing written per row), where a pass of the
// sort reads and rewrites 12-byte pairs.  Most significant digit first, 8 bits per pass.  What has been found so far lives
// in ONE SelectState in device memory: a pass reads it, the one-wave step kernel after it updates it; the host only queues
// the kernels and never waits in between.
//   prefix/mask : the digits found so far (mask = their bits; digits that are constant over all keys never enter it)
//   remaining   : 1-based rank of the wanted row among the rows that match the prefix
//   below       : rows whose processed digits are smaller than the prefix; below + bucket = rows <= the prefix = candidates
//   done        : the candidate range is small enough (stop_cap): later passes return at once
constexpr int kSelectCompactBlock = 4096;

// Count one digit of a wave into the wave's own 256-bin LDS table.  Sorted and low-cardinality keys put the whole wave on
// one bin, and same-address LDS atomics of a wave serialise: two rounds fold the lanes that share the digit of the first
// active lane into one add (ballot + popcount); what is left after that is spread over other bins and adds itself.
__device__ __forceinline__ void select_hist_add(u32 *h, bool active, int digit, int lane) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const u64 m = __ballot(active);
        if (m == 0) return;   // wave-uniform
        const int leader = __ffsll((long long)m) - 1;
        const int d0 = __shfl(digit, leader, 64);
        const u64 same = __ballot(active && digit == d0);
        if (lane == leader) atomicAdd(&h[d0], (u32)__popcll(same));
        if (digit == d0) active = false;
    }
    if (active) atomicAdd(&h[digit], 1u);
}

__global__ void __launch_bounds__(256) select_hist_kernel(const u64 *keys, i64 n, int shift, SelectState *st) {
    __shared__ u32 s_h[4][256];   // one table per wave
    if (st->done) return;         // uniform: the whole grid leaves
    const u64 prefix = st->prefix, mask = st->mask;
    for (int t = threadIdx.x; t < 4 * 256; t += 256) (&s_h[0][0])[t] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    u32 *h = s_h[threadIdx.x >> 6];
    // two rows (16 bytes) per lane; the pair count is padded to whole waves so that every lane of a wave takes part in the ballots
    const i64 npairs = (((n + 1) >> 1) + 63) & ~63ll;
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < npairs; p += stride) {
        const i64 i = 2 * p;
        const bool in0 = i < n, in1 = i + 1 < n;
        u64 k0 = 0, k1 = 0;
        if (in1) {
            const ulonglong2 v = *(const ulonglong2 *)(keys + i);
            k0 = v.x;
            k1 = v.y;
        } else if (in0) {
            k0 = keys[i];
        }
        select_hist_add(h, in0 && (k0 & mask) == prefix, (int)((k0 >> shift) & 255ull), lane);
        select_hist_add(h, in1 && (k1 & mask) == prefix, (int)((k1 >> shift) & 255ull), lane);
    }
    __syncthreads();
    const u32 c = s_h[0][threadIdx.x] + s_h[1][threadIdx.x] + s_h[2][threadIdx.x] + s_h[3][threadIdx.x];
    if (c) atomicAdd(&st->hist[threadIdx.x], c);   // one global atomic per non-empty bin and workgroup
}

// ONE wave: the 256 counts -> the digit that holds the wanted rank, the rank inside it, and whether to stop
__global__ void __launch_bounds__(64) select_step_kernel(SelectState *st, int shift, u64 stop_cap) {
    if (st->done) return;
    const int lane = threadIdx.x;
    u32 c[4];
    u32 sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = st->hist[lane * 4 + j];
        st->hist[lane * 4 + j] = 0;   // ready for the next pass
        sum += c[j];
    }
    const u64 incl = wave_incl_scan<u64>(sum, lane);
    const u64 rem = st->remaining;
    u64 cum = incl - sum;
    if (cum < rem && rem <= incl) {   // exactly one lane (1 <= rem <= rows that match the prefix)
        int j = 0;
        while (j < 3 && rem > cum + c[j]) cum += c[j++];
        st->prefix |= (u64)(lane * 4 + j) << shift;
        st->mask |= 255ull << shift;
        st->remaining = rem - cum;
        st->below += cum;
        st->bucket = c[j];
        st->passes += 1;
        if (st->below + c[j] <= stop_cap) st->done = 1;
    }
}

__device__ __forceinline__ bool select_is_candidate(u64 k, u64 mask, u64 prefix) { return (k & mask) <= prefix; }

// candidates per block of 4096 rows
__global__ void __launch_bounds__(256) select_count_kernel(const u64 *keys, i64 n, const SelectState *st, u32 *counts) {
    __shared__ u32 s_cnt[4];
    const u64 prefix = st->prefix, mask = st->mask;
    const i64 base = (i64)blockIdx.x * kSelectCompactBlock;
    u32 cnt = 0;
#pragma unroll
    for (int r = 0; r < kSelectCompactBlock / 512; ++r) {
        const i64 i = base + r * 512 + 2 * (i64)threadIdx.x;
        if (i + 1 < n) {
            const ulonglong2 v = *(const ulonglong2 *)(keys + i);
            cnt += (select_is_candidate(v.x, mask, prefix) ? 1u : 0u) + (select_is_candidate(v.y, mask, prefix) ? 1u : 0u);
        } else if (i < n) {
            cnt += select_is_candidate(keys[i], mask, prefix) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// row ids of the candidates, in row order: a block without candidates (nearly all of them for a small k) leaves at once
__global__ void __launch_bounds__(256) select_compact_kernel(const u64 *keys, i64 n, const SelectState *st, const u32 *counts, const u32 *offsets,
                                                             u32 *rows_out, i64 capacity) {
    __shared__ u32 s_wave_cnt[4];
    if (counts[blockIdx.x] == 0) return;   // uniform
    const u64 prefix = st->prefix, mask = st->mask;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 base = (i64)blockIdx.x * kSelectCompactBlock;
    u32 running = offsets[blockIdx.x];
    for (int r = 0; r < kSelectCompactBlock / 256; ++r) {
        const i64 i = base + r * 256 + threadIdx.x;
        const bool is = i < n && select_is_candidate(keys[i], mask, prefix);
        const u64 m = __ballot(is);
        const u32 rank = __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
        if (lane == 0) s_wave_cnt[wave] = (u32)__popcll(m);
        __syncthreads();
        u32 pos = running + rank;
        for (int w = 0; w < wave; ++w) pos += s_wave_cnt[w];
        if (is && (i64)pos < capacity) rows_out[pos] = (u32)i;
        running += s_wave_cnt[0] + s_wave_cnt[1] + s_wave_cnt[2] + s_wave_cnt[3];
        __syncthreads();
    }
}

void launch_select_pass(hipStream_t s, const unsigned long long *keys, int64_t n, int shift, SelectState *state, unsigned long long stop_cap) {
    if (n <= 0) return;
    const i64 blocks = (n + 511) / 512;
    hipLaunchKernelGGL(select_hist_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, (const u64 *)keys, (i64)n, shift, state);
    hipLaunchKernelGGL(select_step_kernel, dim3(1), dim3(64), 0, s, state, shift, (u64)stop_cap);
}
int64_t select_compact_blocks(int64_t n) { return (n + kSelectCompactBlock - 1) / kSelectCompactBlock; }
void launch_select_count(hipStream_t s, const unsigned long long *keys, int64_t n, const SelectState *state, uint32_t *counts) {
    if (n <= 0) return;
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)select_compact_blocks(n)), dim3(256), 0, s, (const u64 *)keys, (i64)n, state, counts);
}
void launch_select_compact(hipStream_t s, const unsigned long long *keys, int64_t n, const SelectState *state, const uint32_t *counts,
                           const uint32_t *offsets, uint32_t *rows_out, int64_t capacity) {
    if (n <= 0) return;
    hipLaunchKernelGGL(select_compact_kernel, dim3((unsigned)select_compact_blocks(n)), dim3(256), 0, s, (const u64 *)keys, (i64)n, state, counts, offsets,
                       rows_out, (i64)capacity);
}

}  // namespace qe
