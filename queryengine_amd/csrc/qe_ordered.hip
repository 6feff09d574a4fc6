// qe_ordered.hip -- ordered-set aggregates per group over sorted rows (host side: qe_ordered.cpp).
//
// The rows arrive sorted by (group columns, argument) and marked by launch_win_flags: pstart = a group starts, peer = a run of
// equal argument values starts (the NULL run in front of a group included).  What is left is the step from "sorted rows plus
// two bitmaps" to "one row per group":
//   word ranks   exclusive prefix of the per-word popcounts of a bitmap, so that rank(i) = set bits below i is O(1)
//   compaction   every word scatters the positions of its set bits to prefix[word] + k: the group starts, the run starts
//                (both are the shared bitmap_ranks / bitmap_positions of qe_scan.h, called by qe_ordered.cpp)
//   first valid  inside a group the argument's validity is 0..01..1 (NULL sorts first): one lane per group bisects
//   picks        a u32 source-row list per group that the existing gather turns into the output column (keys,
//                PERCENTILE_DISC, MODE); PERCENTILE_CONT reads its two rows and interpolates; COUNT_DISTINCT is a difference
//                of two ranks; MODE is an integer max over the runs, (length << 32 | ~start) so that the earliest of the
//                longest runs wins
// No look-back, no spin, no loop that waits for another workgroup; every grid is capped and strided; no floating-point value
// goes through an atomic (the one atomic is MODE's u64 max, whose result does not depend on the order of arrival).
#include <hip/hip_runtime.h>

#include "qe_kernels.h"
#include "qe_scan.h"
#include "qe_sort_image.h"

namespace qe {

constexpr u32 kOsaNoRow = 0xFFFFFFFFu;

static unsigned osa_grid(i64 lanes, int max_blocks) {
    const i64 blocks = (lanes + 255) / 256;
    return (unsigned)(blocks < max_blocks ? blocks : max_blocks);
}

// ---- first valid row per group ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) osa_first_valid_kernel(const OsaGroups a, const u64 *valid) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 g = (i64)blockIdx.x * 256 + threadIdx.x; g < a.ngroups; g += stride) {
        i64 lo = a.gstart[g], hi = a.gstart[g + 1];
        if (hi > a.n) hi = a.n;
        if (lo > hi) lo = hi;
        if (valid) {
            while (lo < hi) {   // the bits of [lo, hi) are 0..01..1: at most 32 halvings
                const i64 mid = lo + ((hi - lo) >> 1);
                if (bit_at(valid, mid)) hi = mid;
                else lo = mid + 1;
            }
        }
        a.first[g] = (u32)lo;
    }
}
void launch_osa_first_valid(hipStream_t s, const OsaGroups &g, const unsigned long long *valid) {
    if (g.ngroups <= 0) return;
    hipLaunchKernelGGL(osa_first_valid_kernel, dim3(osa_grid(g.ngroups, kOsaBlocks)), dim3(256), 0, s, g, (const u64 *)valid);
}

// valid values of group g and its first valid position, both kept inside [0, n]
__device__ __forceinline__ void osa_group_values(const OsaGroups &a, i64 g, i64 &first, i64 &count) {
    i64 end = a.gstart[g + 1];
    if (end > a.n) end = a.n;
    first = a.first[g];
    if (first > end) first = end;
    count = end - first;
}

// ---- source-row lists --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) osa_rows_kernel(const OsaGroups a, int kind, double fraction, const u64 *best, u32 *rows_out) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 g = (i64)blockIdx.x * 256 + threadIdx.x; g < a.ngroups; g += stride) {
        i64 at = -1;
        if (kind == QE_OSA_ROWS_KEY) {
            at = a.gstart[g];
        } else if (kind == QE_OSA_ROWS_DISC) {
            i64 first, c;
            osa_group_values(a, g, first, c);
            if (c > 0) {
                i64 k = (i64)ceil(fraction * (double)c) - 1;   // one f64 multiplication
                k = k < 0 ? 0 : k > c - 1 ? c - 1 : k;
                at = first + k;
            }
        } else {
            const u64 b = best[g];
            if (b != 0ull) at = (i64)(kOsaNoRow - (u32)b);
        }
        rows_out[g] = (at >= 0 && at < a.n) ? a.perm[at] : kOsaNoRow;
    }
}
void launch_osa_rows(hipStream_t s, const OsaGroups &g, int kind, double fraction, const unsigned long long *best, uint32_t *rows_out) {
    if (g.ngroups <= 0) return;
    hipLaunchKernelGGL(osa_rows_kernel, dim3(osa_grid(g.ngroups, kOsaBlocks)), dim3(256), 0, s, g, kind, fraction, (const u64 *)best, rows_out);
}

// ---- PERCENTILE_CONT ---------------------------------------------------------------------------------------------------------
// converted as the GROUP BY aggregates convert their input: (double)
__device__ __forceinline__ double osa_value(int type, const void *data, u32 row) {
    switch (type) {
    case QE_DOUBLE: return ((const double *)data)[row];
    case QE_INT64: return (double)((const i64 *)data)[row];
    default: return (double)((const int *)data)[row];
    }
}
__global__ void __launch_bounds__(256) osa_percentile_cont_kernel(const OsaGroups a, int type, const void *data, double fraction, double *out,
                                                                  u64 *out_valid) {
    const i64 padded = (a.ngroups + 63) & ~63ll;   // whole waves for the ballot
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 g = (i64)blockIdx.x * 256 + threadIdx.x; g < padded; g += stride) {
        bool have = false;
        if (g < a.ngroups) {
            i64 first, c;
            osa_group_values(a, g, first, c);
            double r = 0.0;
            if (c > 0) {
                have = true;
                const double h = fraction * (double)(c - 1);
                const double fl = floor(h), ce = ceil(h);
                const double frac = h - fl;
                i64 lo = (i64)fl, hi = (i64)ce;
                lo = lo < 0 ? 0 : lo > c - 1 ? c - 1 : lo;
                hi = hi < 0 ? 0 : hi > c - 1 ? c - 1 : hi;
                const double vlo = osa_value(type, data, a.perm[first + lo]), vhi = osa_value(type, data, a.perm[first + hi]);
                if (frac == 0.0 || __builtin_bit_cast(u64, vlo) == __builtin_bit_cast(u64, vhi)) {
                    r = vlo;
                } else {   // in this order, separately rounded (-ffp-contract=off)
                    const double diff = vhi - vlo;
                    const double step = diff * frac;
                    r = vlo + step;
                }
            }
            out[g] = r;
        }
        const u64 word = __ballot(have);
        if (lane == 0) out_valid[g >> 6] = word;
    }
}
void launch_osa_percentile_cont(hipStream_t s, const OsaGroups &g, int type, const void *data, double fraction, double *out,
                                unsigned long long *out_valid) {
    if (g.ngroups <= 0) return;
    hipLaunchKernelGGL(osa_percentile_cont_kernel, dim3(osa_grid(g.ngroups, kOsaBlocks)), dim3(256), 0, s, g, type, data, fraction, out,
                       (u64 *)out_valid);
}

// ---- COUNT_DISTINCT ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) osa_count_distinct_kernel(const OsaGroups a, const u64 *peer, const u32 *peer_prefix, double *out) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 g = (i64)blockIdx.x * 256 + threadIdx.x; g < a.ngroups; g += stride) {
        i64 first, c;
        osa_group_values(a, g, first, c);
        // the first valid row differs from the row before it (another group, or a NULL): it carries a peer bit
        out[g] = (double)(bitmap_rank(peer, peer_prefix, first + c) - bitmap_rank(peer, peer_prefix, first));
    }
}
void launch_osa_count_distinct(hipStream_t s, const OsaGroups &g, const unsigned long long *peer, const uint32_t *peer_prefix, double *out) {
    if (g.ngroups <= 0) return;
    hipLaunchKernelGGL(osa_count_distinct_kernel, dim3(osa_grid(g.ngroups, kOsaBlocks)), dim3(256), 0, s, g, (const u64 *)peer, peer_prefix, out);
}

// ---- MODE ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) osa_mode_kernel(const OsaGroups a, const u32 *runpos, const u32 *peer_prefix, const u64 *pstart,
                                                       const u32 *pstart_prefix, u64 *best) {
    const i64 nruns = peer_prefix[(a.n + 63) >> 6];
    const i64 padded = (nruns + 63) & ~63ll;   // whole waves for the shuffles
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 r = (i64)blockIdx.x * 256 + threadIdx.x; r < padded; r += stride) {
        u32 g = kOsaNoRow;   // no run: a group of its own that nothing shares
        u64 key = 0ull;      // a run of NULLs keeps 0: it never raises best[]
        if (r < nruns) {
            const i64 p = runpos[r];
            if (p < a.n) {
                const u32 gi = bitmap_rank(pstart, pstart_prefix, p + 1) - 1u;   // row 0 starts a group, so the rank is >= 1
                if ((i64)gi < a.ngroups) {
                    g = gi;
                    i64 first, c;
                    osa_group_values(a, gi, first, c);
                    i64 end = runpos[r + 1];
                    if (end > first + c) end = first + c;   // clipped at the group's end
                    if (p >= first && end > p) key = ((u64)(end - p) << 32) | (u64)(kOsaNoRow - (u32)p);
                }
            }
        }
        // the runs of one group stand side by side: after these steps the first lane of each group in the wave holds its max
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 ok = __shfl_down(key, d, 64);
            const u32 og = __shfl_down(g, d, 64);
            if (lane + d < 64 && og == g && ok > key) key = ok;
        }
        const u32 pg = wave_prev(g);
        const bool head = lane == 0 || pg != g;
        // read first: the atomic is issued only by a wave that would raise the value
        if (head && key != 0ull && best[g] < key) atomicMax(&best[g], key);
    }
}
void launch_osa_mode(hipStream_t s, const OsaGroups &g, const uint32_t *runpos, const uint32_t *peer_prefix, const unsigned long long *pstart,
                     const uint32_t *pstart_prefix, unsigned long long *best) {
    if (g.ngroups <= 0 || g.n <= 0) return;
    hipLaunchKernelGGL(osa_mode_kernel, dim3(osa_grid(g.n, kOsaBlocks)), dim3(256), 0, s, g, runpos, peer_prefix, (const u64 *)pstart, pstart_prefix,
                       (u64 *)best);
}

}  // namespace qe
