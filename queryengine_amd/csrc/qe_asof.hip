// qe_asof.hip -- the kernels of the ASOF join of two results (host side: qe_asof.cpp).
//
// The key columns of the two inputs arrive concatenated (one side's rows, then the other's) and sorted stably by (by columns,
// on); launch_win_flags has marked where a by partition starts.  The order of the concatenation was chosen so that, inside a
// run of equal `on` values, the right rows stand before the left rows exactly when a left row may match them looking back (or
// may not match them looking forward), each side in input order.  What is left is, per left row, the nearest right position:
//   eligible   bit j = the row at sorted position j is valid in every key column; a second bitmap keeps those that are right
//              rows.  With its word ranks and its compacted positions, "the last right row at or before j" is rpos[k - 1] and
//              "the first after j" is rpos[k], k = rank of j.
//   pick       a lane per sorted position; a left row takes its candidate and accepts it when no partition starts between
//              the two positions (two ranks of the start bitmap are equal), and writes match[left row].
//   matched    the match list as a bitmap in left-row order (the INNER form compacts it), and the identity row list.
// A lane per row and a fixed number of loads per lane: no loop over a partition's rows, no atomics, no LDS.  Bitmap words come
// from __ballot and are written by lane 0 of each wave; a lane past row n votes 0, which masks the last partial word.
#include <hip/hip_runtime.h>

#include "qe_kernels.h"
#include "qe_scan.h"
#include "qe_sort_image.h"

namespace qe {

static unsigned asof_grid(i64 lanes) {
    const i64 blocks = (lanes + 255) / 256;
    return (unsigned)(blocks < kAsofBlocks ? blocks : kAsofBlocks);
}

__device__ __forceinline__ bool asof_is_right(const AsofSides &s, i64 row) { return (row < s.nfirst) == (s.right_first != 0); }

// ---- which sorted positions hold a row with a whole key, and which of those a right row ---------------------------------------
__global__ void __launch_bounds__(256) asof_eligible(const AsofEligibleArgs a) {
    const i64 padded = (a.s.n + 63) & ~63ll;   // whole waves for the ballots
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < padded; j += stride) {
        bool ok = false, right = false;
        if (j < a.s.n) {
            const i64 row = a.s.perm[j];
            ok = row < a.s.n;
            for (int k = 0; k < a.nkeys; ++k)
                if (a.validity[k]) ok = ok && bit_at(a.validity[k], row);
            right = ok && asof_is_right(a.s, row);
        }
        const u64 ew = __ballot(ok), rw = __ballot(right);
        if (lane == 0) {
            a.eligible[j >> 6] = ew;
            a.right[j >> 6] = rw;
        }
    }
}
void launch_asof_eligible(hipStream_t s, const AsofEligibleArgs &a) {
    if (a.s.n <= 0) return;
    hipLaunchKernelGGL(asof_eligible, dim3(asof_grid(a.s.n)), dim3(256), 0, s, a);
}

// ---- the match of every left row ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) asof_pick(const AsofPickArgs a) {
    const i64 stride = (i64)gridDim.x * 256;
    i64 nright = a.right_prefix[(a.s.n + 63) >> 6];   // the set bits of `right`: the entries of rpos that were written
    if (nright > a.s.n - a.nleft) nright = a.s.n - a.nleft;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < a.s.n; j += stride) {
        const i64 row = a.s.perm[j];
        if (row >= a.s.n || asof_is_right(a.s, row)) continue;
        const i64 l = row - (a.s.right_first ? a.s.nfirst : 0);
        if (l >= a.nleft) continue;
        u32 found = 0xFFFFFFFFu;
        if (bit_at(a.eligible, j)) {
            const i64 k = bitmap_rank(a.right, a.right_prefix, j);   // j holds a left row: the right rows before it = at or before it
            const i64 at = a.forward ? k : k - 1;
            if (at >= 0 && at < nright) {
                const i64 c = a.rpos[at];
                if (c < a.s.n && (a.forward ? c > j : c < j)) {
                    // no partition start in (c, j] (backward) or (j, c] (forward): the candidate stands in j's partition
                    const i64 lo = a.forward ? j : c, hi = a.forward ? c : j;
                    if (bitmap_rank(a.pstart, a.pstart_prefix, lo + 1) == bitmap_rank(a.pstart, a.pstart_prefix, hi + 1)) {
                        const i64 r = (i64)a.s.perm[c] - (a.s.right_first ? 0 : a.s.nfirst);
                        if (r >= 0 && r < a.s.n - a.nleft) found = (u32)r;
                    }
                }
            }
        }
        a.match[l] = found;
    }
}
void launch_asof_pick(hipStream_t s, const AsofPickArgs &a) {
    if (a.s.n <= 0 || a.nleft <= 0) return;
    hipLaunchKernelGGL(asof_pick, dim3(asof_grid(a.s.n)), dim3(256), 0, s, a);
}

// ---- the matches as a bitmap over the left rows -------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) asof_matched(const u32 *match, i64 nleft, u64 *matched, u32 *identity) {
    const i64 padded = (nleft + 63) & ~63ll;   // whole waves for the ballot
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 l = (i64)blockIdx.x * 256 + threadIdx.x; l < padded; l += stride) {
        const bool hit = l < nleft && match[l] != 0xFFFFFFFFu;
        if (identity && l < nleft) identity[l] = (u32)l;
        const u64 word = __ballot(hit);
        if (lane == 0) matched[l >> 6] = word;
    }
}
void launch_asof_matched(hipStream_t s, const uint32_t *match, int64_t nleft, unsigned long long *matched, uint32_t *identity) {
    if (nleft <= 0) return;
    hipLaunchKernelGGL(asof_matched, dim3(asof_grid(nleft)), dim3(256), 0, s, match, (i64)nleft, (u64 *)matched, identity);
}

}  // namespace qe
