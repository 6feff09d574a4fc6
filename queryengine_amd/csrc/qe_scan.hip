// qe_scan.hip -- the kernels behind qe_scan.h: the one-workgroup carry scan, the three-launch exclusive scan and the
// bitmap compaction.
#include "qe_scan.h"

namespace qe {

namespace {

template <typename T, int THREADS>
__global__ void __launch_bounds__(THREADS) carry_scan_kernel(T *a, i64 n, int nlists, u64 *totals) {
    __shared__ T lds[THREADS / 64];
    const int list = blockIdx.x;
    u64 carry = 0;
    for (i64 b = 0; b < n; b += THREADS) {
        const i64 i = b + threadIdx.x;
        const T x = i < n ? a[i * nlists + list] : (T)0;
        T total;
        const T e = block_excl_scan<T, THREADS>(x, lds, total);
        if (i < n) a[i * nlists + list] = (T)(carry + (u64)e);
        carry += (u64)total;
        __syncthreads();   // every thread has read this trip's wave sums
    }
    if (totals && threadIdx.x == 0) totals[list] = carry;
}

template <typename T, typename Load>
__global__ void __launch_bounds__(kScanBlock) scan_block_sums_kernel(Load load, T *block_sums, i64 n) {
    __shared__ T lds[kScanBlock / 64];
    const i64 i = (i64)blockIdx.x * kScanBlock + threadIdx.x;
    T total;
    (void)block_excl_scan<T, kScanBlock>(i < n ? load(i) : (T)0, lds, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}
template <typename T, typename Load>
__global__ void __launch_bounds__(kScanBlock) scan_final_kernel(Load load, const T *block_offsets, T *out, i64 n) {
    __shared__ T lds[kScanBlock / 64];
    const i64 i = (i64)blockIdx.x * kScanBlock + threadIdx.x;
    T total;
    const T e = block_excl_scan<T, kScanBlock>(i < n ? load(i) : (T)0, lds, total);   // the read of element i ..
    if (i < n) out[i] = block_offsets[blockIdx.x] + e;                                // .. comes before its write: out may alias it
}

// A LANE per bitmap word: lane l walks the set bits of word w0 + l and writes their row ids from prefix[w] on.  The 64
// words of a wave are adjacent and so are their output ranges, so step i of the walk is one store instruction with every
// lane that still has a bit active, all within a few hundred bytes.  (One wave per word -- lanes = bits -- issued a store
// instruction with ~3 active lanes per word at 5 % selectivity: 1.43 ms per 1 B rows.)
// Round 2: when the wave's 64 words hold at most 1024 kept rows (the usual case below ~25 %) the row ids first meet in a 4 KiB
// LDS buffer of the wave and leave in whole 256-byte store instructions: the direct form issues up to max-bits-per-word store
// instructions of 64 lanes x 4 bytes spread over ~12 lines each (0.27 ms per 1 B rows at 10 %).
__global__ void __launch_bounds__(256) bitmap_positions_kernel(const u64 *v, const u64 *k, i64 n, const u32 *prefix, u32 *pos_out, i64 nw,
                                                               i64 capacity, bool sentinel) {
    __shared__ u32 s_buf[4][1024];
    u32 *buf = s_buf[threadIdx.x >> 6];
    const int lane = threadIdx.x & 63;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const i64 nw_pad = (nw + 63) & ~63ll;   // whole waves: the wave-level steps below need every lane
    for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < nw_pad; w += stride) {
        u64 x = w < nw ? keep_word(v, k, w, n) : 0ull;
        u32 pos = w < nw ? prefix[w] : 0u;
        const u32 base = (u32)(w * 64);
        const u32 first = (u32)__builtin_amdgcn_readfirstlane((int)pos);                                   // the wave's words are adjacent
        const u32 cnt = (u32)__popcll(x);
        // total of the wave: an inclusive scan is not needed, offsets are already exclusive -- last valid lane's pos + cnt
        u32 endpos = pos + cnt;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u32 t = (u32)__shfl_xor((int)endpos, o, 64);
            endpos = t > endpos ? t : endpos;
        }
        const u32 total = endpos - first;
        if (total <= 1024u) {
            u32 q = pos - first;
            while (x != 0) {
                buf[q++] = base + (u32)__builtin_ctzll(x);
                x &= x - 1;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            for (u32 j = (u32)lane; j < total; j += 64u)
                if ((i64)first + j < capacity) pos_out[first + j] = buf[j];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        } else {
            while (x != 0) {
                if ((i64)pos < capacity) pos_out[pos] = base + (u32)__builtin_ctzll(x);
                ++pos;
                x &= x - 1;
            }
        }
        if (sentinel && w == 0) {
            const i64 all = prefix[nw];
            if (all < capacity) pos_out[all] = (u32)n;
        }
    }
}

}  // namespace

template <typename T, int THREADS> void launch_carry_scan(hipStream_t s, T *a, int64_t n, int nlists, unsigned long long *totals) {
    if (nlists <= 0) return;
    hipLaunchKernelGGL((carry_scan_kernel<T, THREADS>), dim3((unsigned)nlists), dim3(THREADS), 0, s, a, (i64)n, nlists, (u64 *)totals);
}

template <typename T, typename Load>
void exclusive_scan(hipStream_t s, Load load, T *out, T *block_sums, int64_t n, unsigned long long *total) {
    if (n <= 0) return;
    const int64_t nblocks = scan_blocks(n);
    hipLaunchKernelGGL((scan_block_sums_kernel<T, Load>), dim3((unsigned)nblocks), dim3(kScanBlock), 0, s, load, block_sums, (i64)n);
    launch_carry_scan<T, kScanBlock>(s, block_sums, nblocks, 1, total);
    hipLaunchKernelGGL((scan_final_kernel<T, Load>), dim3((unsigned)nblocks), dim3(kScanBlock), 0, s, load, (const T *)block_sums, out, (i64)n);
}

void bitmap_ranks(hipStream_t s, const uint64_t *v, const uint64_t *k, int64_t n, uint32_t *prefix, uint32_t *block_sums,
                  unsigned long long *total) {
    if (n <= 0) return;
    // one element past the last word, which counts 0: its exclusive sum is the total
    exclusive_scan<u32>(s, KeepWordCount{(const u64 *)v, (const u64 *)k, (i64)n}, prefix, block_sums, (n + 63) / 64 + 1, total);
}

void bitmap_positions(hipStream_t s, const uint64_t *v, const uint64_t *k, int64_t n, const uint32_t *prefix, uint32_t *pos,
                      int64_t capacity, bool sentinel) {
    if (n <= 0) return;
    const i64 nw = (n + 63) / 64, blocks = (nw + 255) / 256;
    hipLaunchKernelGGL(bitmap_positions_kernel, dim3((unsigned)(blocks < 256 * 8 ? blocks : 256 * 8)), dim3(256), 0, s, (const u64 *)v,
                       (const u64 *)k, (i64)n, prefix, pos, nw, (i64)capacity, sentinel);
}

// the instantiations the library and its tests use
template void launch_carry_scan<u32, 256>(hipStream_t, u32 *, int64_t, int, unsigned long long *);
template void launch_carry_scan<u64, 256>(hipStream_t, u64 *, int64_t, int, unsigned long long *);
template void launch_carry_scan<u32, 1024>(hipStream_t, u32 *, int64_t, int, unsigned long long *);
template void launch_carry_scan<u64, 1024>(hipStream_t, u64 *, int64_t, int, unsigned long long *);
template void launch_carry_scan<i64, 1024>(hipStream_t, i64 *, int64_t, int, unsigned long long *);
template void exclusive_scan<u32, ArrayLoad<u32>>(hipStream_t, ArrayLoad<u32>, u32 *, u32 *, int64_t, unsigned long long *);
template void exclusive_scan<i64, ArrayLoad<i64>>(hipStream_t, ArrayLoad<i64>, i64 *, i64 *, int64_t, unsigned long long *);
template void exclusive_scan<u32, KeepWordCount>(hipStream_t, KeepWordCount, u32 *, u32 *, int64_t, unsigned long long *);

}  // namespace qe
