// qe_scan.h -- every plain (non-segmented) prefix sum of the hand-written kernels (kernels: qe_scan.hip).
//
// Device helpers that any .hip file may include, and three launchers:
//   launch_carry_scan   ONE workgroup per list scans a small strided array in place, in trips of THREADS with a carry
//   exclusive_scan      a large array in three launches: block sums, launch_carry_scan over them, final pass
//   bitmap_ranks / bitmap_positions   bitmap -> word ranks -> ascending positions of its set bits
// The launchers are defined in qe_scan.hip for the element types, thread counts and load functors instantiated at its end.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace qe {

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32;

// ---- device helpers --------------------------------------------------------------------------------------------------------
// the value of the lane below (lane 0 keeps its own)
template <typename T> __device__ __forceinline__ T wave_prev(T x) { return __shfl_up(x, 1, 64); }

// inclusive sum over the wave of 64
template <typename T> __device__ __forceinline__ T wave_incl_scan(T x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// Exclusive sum over the workgroup's THREADS values, total = their sum.  lds: THREADS / 64 elements, which the caller may
// reuse (another call included) only behind a __syncthreads() of its own.  Every thread of the workgroup calls.
template <typename T, int THREADS> __device__ __forceinline__ T block_excl_scan(T x, T *lds, T &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const T incl = wave_incl_scan(x, lane);
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    T before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) {
        const T s = lds[w];
        if (w < wave) before += s;
        sum += s;
    }
    total = sum;
    return before + incl - x;
}

// word w of a keep bitmap of n rows: v & k (k null: v alone), the bits past row n cleared; 0 for a word past the last row
__device__ __forceinline__ u64 keep_word(const u64 *v, const u64 *k, i64 w, i64 n) {
    const i64 rem = n - w * 64;
    if (rem <= 0) return 0ull;
    u64 x = v[w];
    if (k) x &= k[w];                               // FilterOperator.kt:20: non-null AND true
    if (rem < 64) x &= (1ull << rem) - 1ull;
    return x;
}

// set bits of `bits` below position i (0 <= i <= n; the bits past n are 0), from the word ranks that bitmap_ranks wrote
__device__ __forceinline__ u32 bitmap_rank(const u64 *bits, const u32 *prefix, i64 i) {
    const int b = (int)(i & 63);
    return prefix[i >> 6] + (b ? (u32)__popcll(bits[i >> 6] & ((1ull << b) - 1ull)) : 0u);
}

// ---- what exclusive_scan sums: element i of an array, or the kept rows of bitmap word i ------------------------------------
template <typename T> struct ArrayLoad {
    const T *p;
    __device__ __forceinline__ T operator()(i64 i) const { return p[i]; }
};
struct KeepWordCount {
    const u64 *v, *k;
    i64 n;
    __device__ __forceinline__ u32 operator()(i64 w) const { return (u32)__popcll(keep_word(v, k, w, n)); }
};

// ---- launchers -----------------------------------------------------------------------------------------------------------
constexpr int kScanBlock = 1024;   // elements per workgroup of exclusive_scan = block sums per trip of its carry scan
inline int64_t scan_blocks(int64_t n) { return (n + kScanBlock - 1) / kScanBlock; }   // entries of block_sums

// Workgroup `list` of nlists replaces a[i * nlists + list], i < n, by the sum of the elements before it in its list, THREADS
// per trip; totals[list] = the list's sum (totals may be null).  The carry and the totals are 64-bit whatever T is.
template <typename T, int THREADS> void launch_carry_scan(hipStream_t s, T *a, int64_t n, int nlists, unsigned long long *totals);

// out[i] = load(0) + .. + load(i - 1), i < n; *total = the sum of all n (total may be null).  block_sums: scan_blocks(n)
// elements of scratch.  out may be the array that load reads: the block-sum pass only reads, and in the final pass every
// thread reads its own element before it writes it.  Sums are exact below the range of T.
template <typename T, typename Load>
void exclusive_scan(hipStream_t s, Load load, T *out, T *block_sums, int64_t n, unsigned long long *total);

// Word ranks of the keep bitmap v & k (k may be null) of n rows: prefix[w] = kept rows in the words before w, for w <=
// ceil(n / 64) -- one entry more than there are words, the last is the total -- so that rank(i) = prefix[i >> 6] +
// popc(word & low_mask(i)).  block_sums: scan_blocks(ceil(n / 64) + 1) u32 of scratch.  *total as in exclusive_scan.
void bitmap_ranks(hipStream_t s, const uint64_t *v, const uint64_t *k, int64_t n, uint32_t *prefix, uint32_t *block_sums,
                  unsigned long long *total);
// pos[r] = row of the r-th kept row (ascending), from the prefix that bitmap_ranks wrote; sentinel: also pos[total] = n.
// Only entries below `capacity` are written.
void bitmap_positions(hipStream_t s, const uint64_t *v, const uint64_t *k, int64_t n, const uint32_t *prefix, uint32_t *pos,
                      int64_t capacity, bool sentinel);

}  // namespace qe
