// qe_range.cpp -- host side of the range join of two results (kernels: qe_range.hip): for every left row ALL
// right rows of the same by tuple whose `on` value lies between the left row's two bounds.  The key columns of the two sides
// are sorted as one by (by.., value) (TwoSidedKeys, qe_exec.h) twice, once with the lower and once with the upper bound as the
// left rows' value; in each sort a left row reads off how many eligible right rows stand before it.  Both numbers index one
// list of the eligible right rows, so their difference is the row's match count; a 64-bit scan of the counts and a
// load-balanced expansion turn them into row pairs for the output step of every join (emit_joined).
#include "qe_exec.h"
#include "qe_scan.h"

namespace qe {
namespace {

// One of the two sorts: ord[l] = the eligible right rows that stand before left row l in the order (by.., value), where the
// left rows' value is column `left_value` and, among equal keys, the right rows stand first when right_first; 0xFFFFFFFF for a
// left row without a whole key.  rlist (may be null): the eligible right rows in that order.  Everything this needs besides
// the two outputs is released before it returns.
void sorted_ordinals(qe_ctx *ctx, const TwoSidedCall &q, int32_t left_value, int32_t right_on, bool right_first, uint32_t *ord, uint32_t *rlist) {
    PoolScratch sc(ctx);
    TwoSidedKeys keys(ctx, sc, q, left_value, right_on, right_first);
    keys.mark();
    RangeOrdinalArgs oa{};
    oa.s = keys.sides;
    oa.nleft = keys.nl;
    oa.eligible = keys.eligible;
    oa.right = keys.right;
    oa.right_prefix = keys.right_prefix;
    oa.ord = ord;
    oa.rlist = rlist;
    launch_range_ordinals(ctx->stream, oa);
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));   // the key result and this sort's scratch go back to the pool now
}

qe_result *run_range(qe_ctx *ctx, const TwoSidedCall &q, int32_t left_lo, int32_t left_hi, int32_t right_on, int32_t lo_strict, int32_t hi_strict) {
    check_call(q, kJoinsAll, (lo_strict != 0 && lo_strict != 1) || (hi_strict != 0 && hi_strict != 1) ? "a strict flag is 0 or 1" : nullptr);
    const ValueColumn values[3] = {{false, left_lo, "left lo"}, {false, left_hi, "left hi"}, {true, right_on, "right on"}};
    check_sides(q, values, 3);
    need_device(ctx);
    const int64_t nl = q.left->count, nr = q.right->count;
    // RIGHT / FULL: the HEAD is the INNER / LEFT output, the TAIL the right rows that no left row matched
    const bool outer = q.join_type == QE_JOIN_RIGHT || q.join_type == QE_JOIN_FULL;
    const bool left_join = q.join_type == QE_JOIN_LEFT || q.join_type == QE_JOIN_FULL, pairs = left_join || outer || q.join_type == QE_JOIN_INNER;

    PoolScratch sc(ctx);
    int64_t nout = 0, nemit = 0, longest = 0, tail = 0;
    uint32_t *ord_lo = nullptr, *cnt = nullptr, *rlist = nullptr, *keep_prefix = nullptr, *cover = nullptr, *tail_prefix = nullptr;
    long long *offset = nullptr;
    unsigned long long *keep = nullptr, *unmatched = nullptr;
    unsigned long long *d_ctl = (unsigned long long *)sc.alloc(32);   // [0] output rows of the head, [1] longest (u32), [2] kept left rows, [3] tail rows
    QE_HIP(hipMemsetAsync(d_ctl, 0, 32, ctx->stream));
    if (outer && nr > 0) {   // the marks over the right rows, and (both sides there) the difference array over the list positions
        unmatched = (unsigned long long *)sc.alloc(bitmap_bytes(nr));
        QE_HIP(hipMemsetAsync(unmatched, 0, bitmap_bytes(nr), ctx->stream));
        if (nl > 0) {
            cover = (uint32_t *)sc.alloc((size_t)(nr + 1) * 4);
            QE_HIP(hipMemsetAsync(cover, 0, (size_t)(nr + 1) * 4, ctx->stream));
        }
    }
    if (nl > 0) {
        // ---- 1. the two ordinals of every left row.  Ties fall by the order of the concatenation, as in the ASOF join: an
        // inclusive lower end counts only the right rows BELOW lo (left rows first), an inclusive upper end also those equal
        // to hi (right rows first); a strict end the other way round ----
        ord_lo = (uint32_t *)sc.alloc((size_t)nl * 4);
        uint32_t *ord_hi = (uint32_t *)sc.alloc((size_t)nl * 4);
        if (nr > 0) {
            if (pairs) rlist = (uint32_t *)sc.alloc((size_t)nr * 4);
            sorted_ordinals(ctx, q, left_lo, right_on, lo_strict != 0, ord_lo, rlist);
            sorted_ordinals(ctx, q, left_hi, right_on, hi_strict == 0, ord_hi, nullptr);
        } else {   // nothing to match: no sort
            QE_HIP(hipMemsetAsync(ord_lo, 0xFF, (size_t)nl * 4, ctx->stream));
            QE_HIP(hipMemsetAsync(ord_hi, 0xFF, (size_t)nl * 4, ctx->stream));
        }

        // ---- 2. the counts, the rows every left row emits and their 64-bit offsets; the rows with (SEMI, INNER) or without
        // (ANTI) a match as a bitmap with its ranks ----
        cnt = (uint32_t *)sc.alloc((size_t)nl * 4);
        keep = (unsigned long long *)sc.alloc(bitmap_bytes(nl));
        if (pairs) offset = (long long *)sc.alloc((size_t)nl * 8);
        RangeCountArgs ca{};
        ca.nleft = nl;
        ca.nright = nr;
        ca.cover = cover;
        ca.left_join = left_join ? 1 : 0;
        ca.anti = q.join_type == QE_JOIN_ANTI ? 1 : 0;
        ca.ord_lo = ord_lo;
        ca.ord_hi = ord_hi;
        ca.cnt = cnt;
        ca.emit = offset;
        ca.keep = keep;
        ca.longest = (uint32_t *)(d_ctl + 1);
        launch_range_counts(ctx->stream, ca);
        if (pairs) {
            long long *sums = (long long *)sc.alloc((size_t)scan_blocks(nl) * 8);
            exclusive_scan<i64>(ctx->stream, ArrayLoad<i64>{offset}, offset, sums, nl, d_ctl);   // in place
        }
        if (!left_join) {   // LEFT: every left row emits, nothing to compact
            uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(bitmap_words(nl) + 1) * 4);
            keep_prefix = (uint32_t *)sc.alloc((size_t)(bitmap_words(nl) + 1) * 4);
            bitmap_ranks(ctx->stream, (const uint64_t *)keep, nullptr, nl, keep_prefix, sums, d_ctl + (pairs ? 2 : 0));
        }
    }
    if (unmatched) {
        // ---- 2a. RIGHT / FULL: difference array -> cover counts -> marks -> the unmatched right rows and their ranks ----
        if (cover) {
            uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(nr + 1) * 4);
            exclusive_scan<u32>(ctx->stream, ArrayLoad<u32>{cover}, cover, sums, nr + 1, nullptr);   // in place
            RangeMarkArgs ma{};
            ma.nright = nr;
            ma.scanned = cover;
            ma.rlist = rlist;
            ma.matched = unmatched;
            launch_range_mark(ctx->stream, ma);
        }
        uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(bitmap_words(nr) + 1) * 4);
        tail_prefix = (uint32_t *)sc.alloc((size_t)(bitmap_words(nr) + 1) * 4);
        launch_join_unmatched(ctx->stream, unmatched, nr);
        bitmap_ranks(ctx->stream, (const uint64_t *)unmatched, nullptr, nr, tail_prefix, sums, d_ctl + 3);
    }
    if (nl > 0 || unmatched) {
        unsigned long long h_ctl[4] = {0, 0, 0, 0};
        QE_HIP(hipMemcpyAsync(h_ctl, d_ctl, 32, hipMemcpyDeviceToHost, ctx->stream));   // the one read-back besides the sorts' own
        QE_HIP(hipGetLastError());
        QE_HIP(hipStreamSynchronize(ctx->stream));
        nout = (int64_t)h_ctl[0];   // at most 2^32 rows of at most 2^32 matches: fits; an output too large for the device is
                                    // reported by the pool below (QE_ERR_OOM)
        longest = (int64_t)(uint32_t)h_ctl[1];
        nemit = left_join ? nl : pairs ? (int64_t)h_ctl[2] : nout;
        tail = (int64_t)h_ctl[3];
        if (tail < 0 || tail > nr) fail(QE_ERR_INTERNAL, std::string(q.who) + ": " + std::to_string(tail) + " unmatched of " + std::to_string(nr) + " right rows");
        if (nout < 0 || nemit < 0 || nemit > nl || longest > nr || (nout > 0 && nemit == 0) || (!pairs && nout > nl))
            fail(QE_ERR_INTERNAL, std::string(q.who) + ": " + std::to_string(nout) + " output rows from " + std::to_string(nemit) + " of " +
                                      std::to_string(nl) + " left rows, longest " + std::to_string(longest));
    }

    // ---- 3. the row lists: the kept left rows (SEMI / ANTI), or the expansion into pairs (INNER / LEFT) ----
    const int64_t nrows = nout + tail;
    ResultPtr res = new_result(ctx, nrows);
    uint32_t *lrows = nullptr, *rrows = nullptr;
    if (nrows > 0) {
        lrows = (uint32_t *)sc.alloc((size_t)nrows * 4);
        if (!pairs) {
            bitmap_positions(ctx->stream, (const uint64_t *)keep, nullptr, nl, keep_prefix, lrows, nout, false);
        } else {
            rrows = (uint32_t *)sc.alloc((size_t)nrows * 4);
            RangeExpandArgs xa{};
            xa.total = nout;
            xa.nemit = nemit;
            xa.nleft = nl;
            xa.nright = nr;
            xa.eoff = offset;
            if (!left_join) {   // the emitting left rows and their offsets, compacted: a tile of output rows meets at most a tile of them
                uint32_t *erow = (uint32_t *)sc.alloc((size_t)nemit * 4);
                long long *eoff = (long long *)sc.alloc((size_t)nemit * 8);
                bitmap_positions(ctx->stream, (const uint64_t *)keep, nullptr, nl, keep_prefix, erow, nemit, false);
                launch_gather_rows(ctx->stream, 8, offset, erow, nemit, eoff);
                xa.erow = erow;
                xa.eoff = eoff;
            }
            xa.cnt = cnt;
            xa.ord_lo = ord_lo;
            xa.rlist = rlist;
            xa.lrow = lrows;
            xa.rrow = rrows;
            launch_range_expand(ctx->stream, xa);   // (no launch for an empty head)
        }
        if (tail > 0) {   // the tail extends the two lists: no left row, the unmatched right rows ascending
            QE_HIP(hipMemsetAsync(lrows + nout, 0xFF, (size_t)tail * 4, ctx->stream));
            bitmap_positions(ctx->stream, (const uint64_t *)unmatched, nullptr, nr, tail_prefix, rrows + nout, tail, false);
        }
    }

    // ---- 4. the output: the listed left columns by the left rows, the listed right columns by their matches ----
    emit_joined(ctx, res.get(), nrows, q.left->cols, q.left_out, q.nleft_out, lrows, q.right->cols, q.right_out, q.nright_out, rrows, outer,
                left_join, kGatherBlocksWide);
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));   // the scratch goes back to the pool now
    ctx->range_stats.store(nl, nr, nrows, longest);
    if (outer) ctx->outer_stats.store(2, nout, tail, nr - tail);
    return res.release();
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int32_t qe_result_range_join(qe_ctx *ctx, const qe_result *left, const qe_result *right, const int32_t *left_by, const int32_t *right_by,
                             int32_t nby, int32_t left_lo, int32_t left_hi, int32_t right_on, int32_t lo_strict, int32_t hi_strict,
                             int32_t join_type, const int32_t *left_out, int32_t nleft_out, const int32_t *right_out, int32_t nright_out,
                             qe_result **out) {
    if (out) *out = nullptr;
    if (!ctx || !left || !right || !out) return QE_ERR_INVALID_ARG;
    const TwoSidedCall q{"qe_result_range_join", left, right, left_by, right_by, nby, left_out, right_out, nleft_out, nright_out, join_type};
    return guarded(ctx, [&] { *out = run_range(ctx, q, left_lo, left_hi, right_on, lo_strict, hi_strict); });
}

int32_t qe_ctx_last_range_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::range_stats, out); }

}  // extern "C"
