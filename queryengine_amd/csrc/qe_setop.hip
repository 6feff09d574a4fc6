// qe_setop.hip -- the kernels of UNION / INTERSECT / EXCEPT [ALL] over two results (host side: qe_setop.cpp).
//
// The two inputs arrive concatenated (left rows, then right rows) and sorted stably by every column; launch_win_flags has
// marked where a tuple starts.  What is left is to say, per sorted position, whether its row is one of the k copies of its
// tuple that the operation keeps:
//   translate   the right side's STRING codes go through a host-built table into the merged dictionary, before the sort
//   side bits   bit j = the row at sorted position j is a left row; with its word ranks, cL of any range is two lookups
//   keep        position j finds its tuple [s, e) through the rank of the start bitmap and the compacted starts, takes cL
//               and cR = e - s - cL, and keeps itself when it is among the first k rows of the tuple.  The sort is stable
//               and started from the identity, so those are the tuple's left rows in input order, then its right rows.
// A lane per row and a fixed number of loads per lane: no loop over a tuple's rows, no atomics, no LDS.  Bitmap words come
// from __ballot and are written by lane 0 of each wave; a lane past row n votes 0, which masks the last partial word.
#include <hip/hip_runtime.h>

#include "qe_kernels.h"
#include "qe_scan.h"

namespace qe {

static unsigned setop_grid(i64 lanes) {
    const i64 blocks = (lanes + 255) / 256;
    return (unsigned)(blocks < kSetopBlocks ? blocks : kSetopBlocks);
}

// ---- right-side STRING codes into the merged dictionary -----------------------------------------------------------------------
__global__ void __launch_bounds__(256) setop_translate_codes(const int *codes, i64 n, const int *table, int ncodes, int *out) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int c = codes[i];
        out[i] = (u32)c < (u32)ncodes ? table[c] : 0;
    }
}
void launch_setop_translate_codes(hipStream_t s, const int *codes, int64_t n, const int *table, int ncodes, int *out) {
    if (n <= 0) return;
    hipLaunchKernelGGL(setop_translate_codes, dim3(setop_grid(n)), dim3(256), 0, s, codes, (i64)n, table, ncodes, out);
}

// ---- which sorted positions hold a left row --------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) setop_side_bits(const u32 *perm, i64 n, i64 nleft, u64 *side) {
    const i64 padded = (n + 63) & ~63ll;   // whole waves for the ballot
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < padded; j += stride) {
        const bool left = j < n && (i64)perm[j] < nleft;
        const u64 word = __ballot(left);
        if (lane == 0) side[j >> 6] = word;
    }
}
void launch_setop_side_bits(hipStream_t s, const uint32_t *perm, int64_t n, int64_t nleft, unsigned long long *side) {
    if (n <= 0) return;
    hipLaunchKernelGGL(setop_side_bits, dim3(setop_grid(n)), dim3(256), 0, s, perm, (i64)n, (i64)nleft, (u64 *)side);
}

// ---- the keep bitmap -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) setop_keep(const SetopKeepArgs a) {
    const i64 padded = (a.n + 63) & ~63ll;   // whole waves for the ballot
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < padded; j += stride) {
        bool keep = false;
        if (j < a.n) {
            i64 g = (i64)bitmap_rank(a.pstart, a.pstart_prefix, j + 1) - 1;   // row 0 starts a tuple, so the rank is >= 1
            g = g < 0 ? 0 : g > a.ntuples - 1 ? a.ntuples - 1 : g;
            i64 s = a.gstart[g], e = a.gstart[g + 1];
            if (e > a.n) e = a.n;
            if (s > j) s = j;
            if (e <= j) e = j + 1;
            const i64 cl = (i64)bitmap_rank(a.side, a.side_prefix, e) - (i64)bitmap_rank(a.side, a.side_prefix, s);
            const i64 cr = e - s - cl;
            i64 k;
            if (a.op == QE_SET_UNION) k = a.all ? cl + cr : 1;
            else if (a.op == QE_SET_INTERSECT) k = a.all ? (cl < cr ? cl : cr) : (cl > 0 && cr > 0 ? 1 : 0);
            else k = a.all ? (cl > cr ? cl - cr : 0) : (cl > 0 && cr == 0 ? 1 : 0);
            keep = j - s < k;
        }
        const u64 word = __ballot(keep);
        if (lane == 0) a.keep[j >> 6] = word;
    }
}
void launch_setop_keep(hipStream_t s, const SetopKeepArgs &a) {
    if (a.n <= 0 || a.ntuples <= 0) return;
    hipLaunchKernelGGL(setop_keep, dim3(setop_grid(a.n)), dim3(256), 0, s, a);
}

}  // namespace qe
