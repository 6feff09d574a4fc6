// qe_range.hip -- the kernels of the range join of two results (host side: qe_range.cpp).
//
// The key columns of the two inputs arrive concatenated and sorted stably by (by columns, value), twice: once with the left
// rows' lower bound as their value, once with their upper bound; the right rows carry `on` both times.  launch_asof_eligible
// (qe_asof.hip) has marked the positions whose row has a whole key and the right rows among them, and bitmap_ranks the words.
//   ordinals   a lane per sorted position; a left row takes the number of eligible right rows before it (its ORDINAL), an
//              eligible right row puts itself at its own ordinal of the list R.  The eligible right rows stand in the same
//              order in both sorts, so the two ordinals of a left row index one list and its matches are R[lo .. hi).
//   counts     a lane per left row: cnt = hi - lo (0 without a whole key, or when the interval is empty), the rows it emits,
//              a keep bitmap for SEMI / ANTI and for compacting the emitting rows, and the largest cnt.
//   expand     a workgroup per tile of kRangeExpandTile consecutive OUTPUT rows.  The first output rows of the emitting left
//              rows ascend strictly, so at most kRangeExpandTile + 1 of them reach into a tile: they are staged in LDS relative
//              to the tile, and every lane finds the left row of its output row by a binary search there.  No lane walks a
//              left row's matches: the work per output row is the search, whatever the counts are, and the stores of a wave
//              are 256 contiguous bytes.
//   cover      RIGHT / FULL only.  The matched right rows are the union of the intervals R[lo .. hi) of the left rows.  `counts`
//              adds +1 at lo and -1 at hi of every left row with a match into a zeroed DIFFERENCE ARRAY over the list positions:
//              u32, modulo 2^32 -- a position is covered by at most nleft < 2^32 intervals, so the scanned value is exact.  The
//              shared exclusive scan turns it into the cover count of every position, and `mark` sets the bit of right row R[p]
//              for every covered p in a bitmap over right rows (two positions may share a word: an integer OR).  Complemented
//              (launch_join_unmatched), ranked and compacted it is the tail of the output.
// Bitmap words come from __ballot and are written by lane 0 of each wave; a lane past the last row votes 0.  The atomics are
// the integer max of the counts, which feeds the stats only, and under RIGHT / FULL the integer adds of the difference array
// and the integer ORs of the marks: the final value of each is the same in whatever order they arrive.
#include <hip/hip_runtime.h>

#include "qe_kernels.h"
#include "qe_scan.h"
#include "qe_sort_image.h"

namespace qe {

static constexpr u32 kNoRow = 0xFFFFFFFFu;

static unsigned range_grid(i64 lanes) {
    const i64 blocks = (lanes + 255) / 256;
    return (unsigned)(blocks < kRangeBlocks ? blocks : kRangeBlocks);
}

// ---- the ordinal of every left row, and the eligible right rows in sorted order -------------------------------------------------
__global__ void __launch_bounds__(256) range_ordinals(const RangeOrdinalArgs a) {
    const i64 stride = (i64)gridDim.x * 256;
    const i64 nright = a.s.n - a.nleft;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < a.s.n; j += stride) {
        const i64 row = a.s.perm[j];
        if (row >= a.s.n) continue;
        const u32 k = bitmap_rank(a.right, a.right_prefix, j);   // the eligible right rows before position j
        if ((row < a.s.nfirst) == (a.s.right_first != 0)) {
            const i64 r = row - (a.s.right_first ? 0 : a.s.nfirst);
            if (a.rlist && bit_at(a.right, j) && r < nright && (i64)k < nright) a.rlist[k] = (u32)r;
        } else {
            const i64 l = row - (a.s.right_first ? a.s.nfirst : 0);
            if (l < a.nleft) a.ord[l] = bit_at(a.eligible, j) ? k : kNoRow;
        }
    }
}
void launch_range_ordinals(hipStream_t s, const RangeOrdinalArgs &a) {
    if (a.s.n <= 0 || a.nleft <= 0) return;
    hipLaunchKernelGGL(range_ordinals, dim3(range_grid(a.s.n)), dim3(256), 0, s, a);
}

// ---- matches per left row -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) range_counts(const RangeCountArgs a) {
    const i64 padded = (a.nleft + 63) & ~63ll;   // whole waves for the ballot
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    u32 most = 0;
    for (i64 l = (i64)blockIdx.x * 256 + threadIdx.x; l < padded; l += stride) {
        const bool in = l < a.nleft;
        u32 c = 0;
        if (in) {
            const u32 lo = a.ord_lo[l], hi = a.ord_hi[l];
            if (lo != kNoRow && hi != kNoRow && hi > lo) c = hi - lo;
            a.cnt[l] = c;
            if (a.cover && c != 0 && (i64)hi <= a.nright) {   // RIGHT / FULL (the same in every lane): [lo, hi) is covered once more
                atomicAdd(a.cover + lo, 1u);
                atomicAdd(a.cover + hi, 0xFFFFFFFFu);   // -1 modulo 2^32
            }
            if (a.emit) a.emit[l] = (a.left_join && c == 0) ? 1ll : (i64)c;
        }
        most = c > most ? c : most;
        const u64 word = __ballot(in && ((c != 0) != (a.anti != 0)));
        if (lane == 0) a.keep[l >> 6] = word;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u32 t = (u32)__shfl_xor((int)most, o, 64);
        most = t > most ? t : most;
    }
    if (lane == 0 && most != 0) atomicMax(a.longest, most);   // stats only: the order of arrival does not show
}
void launch_range_counts(hipStream_t s, const RangeCountArgs &a) {
    if (a.nleft <= 0) return;
    hipLaunchKernelGGL(range_counts, dim3(range_grid(a.nleft)), dim3(256), 0, s, a);
}

// ---- RIGHT / FULL: the covered list positions as marks over the right rows ---------------------------------------------------------
__global__ void __launch_bounds__(256) range_mark(const RangeMarkArgs a) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < a.nright; p += stride) {
        if (a.scanned[p + 1] == 0) continue;   // the sum of the differences up to and including p: the intervals that hold p
        const i64 r = a.rlist[p];              // (a covered position is below the number of eligible right rows: rlist[p] is written)
        if (r < a.nright) atomicOr(a.matched + (r >> 6), 1ull << (r & 63));
    }
}
void launch_range_mark(hipStream_t s, const RangeMarkArgs &a) {
    if (a.nright <= 0) return;
    hipLaunchKernelGGL(range_mark, dim3(range_grid(a.nright)), dim3(256), 0, s, a);
}

// ---- the expansion of the counts into (left row, right row) pairs ----------------------------------------------------------------
__global__ void __launch_bounds__(256) range_expand(const RangeExpandArgs a) {
    constexpr int T = kRangeExpandTile;
    __shared__ int s_start[T + 1];   // first output row of the emitting rows e0, e0 + 1, .., relative to the tile; T: not in this tile
    const i64 ntiles = (a.total + T - 1) / T;
    for (i64 tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const i64 o0 = tile * T;
        // e0 = the last emitting row that starts at or before o0 (eoff[0] == 0: there is one); the same in every lane
        i64 lo = 0, hi = a.nemit;
        while (hi - lo > 1) {
            const i64 mid = lo + ((hi - lo) >> 1);
            if (a.eoff[mid] <= o0) lo = mid;
            else hi = mid;
        }
        const i64 e0 = lo;
        const i64 k0 = o0 - a.eoff[e0];   // matches of e0 that earlier tiles hold
        for (int i = threadIdx.x; i <= T; i += 256) {
            const i64 e = e0 + i;
            int v = T;
            if (e < a.nemit) {
                const i64 d = a.eoff[e] - o0;
                v = d < 0 ? 0 : d > T ? T : (int)d;
            }
            s_start[i] = v;
        }
        __syncthreads();
        for (int s = threadIdx.x; s < T; s += 256) {   // lane = output row: coalesced stores
            const i64 o = o0 + s;
            if (o >= a.total) break;
            // the last i with s_start[i] <= s.  s_start[0] == 0, and s_start ascends strictly below T, so s_start[i] >= i: i <= s
            int b = 0, t = s + 1;
            while (t - b > 1) {
                const int mid = (b + t) >> 1;
                if (s_start[mid] <= s) b = mid;
                else t = mid;
            }
            const i64 e = e0 + b;
            const i64 k = b == 0 ? k0 + s : (i64)(s - s_start[b]);
            u32 l = kNoRow, r = kNoRow;
            if (e < a.nemit) {
                const i64 row = a.erow ? (i64)a.erow[e] : e;
                if (row < a.nleft) {
                    l = (u32)row;
                    const i64 c = a.cnt[row];
                    const i64 at = (i64)a.ord_lo[row] + k;
                    if (k >= 0 && k < c && at < a.nright) r = a.rlist[at];
                }
            }
            a.lrow[o] = l;
            a.rrow[o] = r;
        }
        __syncthreads();   // the next tile restages s_start
    }
}
void launch_range_expand(hipStream_t s, const RangeExpandArgs &a) {
    if (a.total <= 0 || a.nemit <= 0) return;
    const i64 ntiles = (a.total + kRangeExpandTile - 1) / kRangeExpandTile;
    hipLaunchKernelGGL(range_expand, dim3((unsigned)(ntiles < kRangeBlocks ? ntiles : kRangeBlocks)), dim3(256), 0, s, a);
}

}  // namespace qe
