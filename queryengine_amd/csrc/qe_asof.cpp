// qe_asof.cpp -- host side of the ASOF join of two results (kernels: qe_asof.hip): for every left row the one
// right row of the same by tuple whose `on` value is nearest at or before (after) it.  The key columns of the two sides are
// sorted once as one by (by.., on) (TwoSidedKeys, qe_exec.h) and marked with the partition starts; two kernels find, per left
// row, the nearest eligible right position inside its partition, and the output step of every join (emit_joined) gathers the rows.
#include "qe_exec.h"
#include "qe_scan.h"

namespace qe {
namespace {

qe_result *run_asof(qe_ctx *ctx, const TwoSidedCall &q, int32_t left_on, int32_t right_on, int32_t direction, int32_t strict) {
    check_call(q, kJoinsPairs,
               direction != QE_ASOF_BACKWARD && direction != QE_ASOF_FORWARD ? "unknown direction" : strict != 0 && strict != 1 ? "strict is 0 or 1" : nullptr);
    const ValueColumn on[2] = {{false, left_on, "left on"}, {true, right_on, "right on"}};
    check_sides(q, on, 2);
    need_device(ctx);
    const int64_t nl = q.left->count, nr = q.right->count, n = nl + nr;
    const bool forward = direction == QE_ASOF_FORWARD, inner = q.join_type == QE_JOIN_INNER;
    int64_t stats[4] = {nl, nr, 0, 0};

    PoolScratch sc(ctx);
    uint32_t *match = nullptr;            // per left row: its right row or 0xFFFFFFFF
    unsigned long long *matched = nullptr;
    uint32_t *matched_prefix = nullptr, *identity = nullptr;
    int64_t nmatched = 0;
    std::unique_ptr<TwoSidedKeys> keys;   // released with the scratch, after the last kernel
    if (n > 0) {
        // ---- 1. one stable sort of both sides over (by.., on).  The right rows go first where a left row may match an equal
        // `on` looking back, or may not match it looking forward ----
        keys.reset(new TwoSidedKeys(ctx, sc, q, left_on, right_on, forward == (strict != 0)));

        // ---- 2. the partition starts through the same row ids ----
        const int64_t nwords = bitmap_words(n);
        unsigned long long *pstart = (unsigned long long *)sc.alloc(bitmap_bytes(n));
        unsigned long long *peer = (unsigned long long *)sc.alloc(bitmap_bytes(n));   // the runs of equal `on`: not read
        unsigned long long *d_count = (unsigned long long *)sc.alloc(16);   // [0] partitions, [1] matched left rows
        uint32_t *pstart_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
        keys->runs.flag(q.nby, pstart, peer, d_count);
        keys->runs.rank_starts(pstart, pstart_prefix, keys->sums);

        // ---- 3. the rows with a whole key, and the right rows among them ----
        keys->mark();

        // ---- 4. the pick, and the matches as a bitmap over the left rows ----
        if (nl > 0) {
            uint32_t *rpos = (uint32_t *)sc.alloc((size_t)(nr + 1) * 4);   // the eligible right rows are at most nr; the kernel reads their number
            match = (uint32_t *)sc.alloc((size_t)nl * 4);
            matched = (unsigned long long *)sc.alloc(bitmap_bytes(nl));
            matched_prefix = (uint32_t *)sc.alloc((size_t)(bitmap_words(nl) + 1) * 4);
            if (!inner) identity = (uint32_t *)sc.alloc((size_t)nl * 4);
            bitmap_positions(ctx->stream, (const uint64_t *)keys->right, nullptr, n, keys->right_prefix, rpos, nr, false);
            AsofPickArgs pa{};
            pa.s = keys->sides;
            pa.forward = forward ? 1 : 0;
            pa.nleft = nl;
            pa.eligible = keys->eligible;
            pa.right = keys->right;
            pa.pstart = pstart;
            pa.right_prefix = keys->right_prefix;
            pa.pstart_prefix = pstart_prefix;
            pa.rpos = rpos;
            pa.match = match;
            launch_asof_pick(ctx->stream, pa);
            launch_asof_matched(ctx->stream, match, nl, matched, identity);
            bitmap_ranks(ctx->stream, (const uint64_t *)matched, nullptr, nl, matched_prefix, keys->sums, d_count + 1);
        }
        unsigned long long h_count[2] = {0, 0};
        QE_HIP(hipMemcpyAsync(h_count, d_count, 16, hipMemcpyDeviceToHost, ctx->stream));   // the one read-back besides the sort's own
        QE_HIP(hipGetLastError());
        QE_HIP(hipStreamSynchronize(ctx->stream));
        const int64_t G = checked_runs(q.who, h_count[0], "partitions", n);
        nmatched = (int64_t)h_count[1];
        if (nmatched < 0 || nmatched > nl) fail(QE_ERR_INTERNAL, std::string(q.who) + ": matched " + std::to_string(nmatched) + " of " + std::to_string(nl) + " left rows");
        stats[3] = G;
        stats[2] = nmatched;
    }

    // ---- 5. the output: the listed left columns by the kept left rows, the listed right columns by their matches ----
    const int64_t nout = inner ? nmatched : nl;
    ResultPtr res = new_result(ctx, nout);
    const uint32_t *lrows = identity, *rrows = match;
    if (inner && nout > 0) {
        uint32_t *kept = (uint32_t *)sc.alloc((size_t)nout * 4), *theirs = (uint32_t *)sc.alloc((size_t)nout * 4);
        bitmap_positions(ctx->stream, (const uint64_t *)matched, nullptr, nl, matched_prefix, kept, nout, false);
        launch_gather_rows(ctx->stream, 4, match, kept, nout, theirs);
        lrows = kept;
        rrows = theirs;
    }
    emit_joined(ctx, res.get(), nout, q.left->cols, q.left_out, q.nleft_out, lrows, q.right->cols, q.right_out, q.nright_out, rrows, false, !inner,
                kGatherBlocks);
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));   // the key result and the scratch go back to the pool now
    ctx->asof_stats.store(stats);
    return res.release();
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int32_t qe_result_asof_join(qe_ctx *ctx, const qe_result *left, const qe_result *right, const int32_t *left_by, const int32_t *right_by,
                            int32_t nby, int32_t left_on, int32_t right_on, int32_t direction, int32_t strict, int32_t join_type,
                            const int32_t *left_out, int32_t nleft_out, const int32_t *right_out, int32_t nright_out, qe_result **out) {
    if (out) *out = nullptr;
    if (!ctx || !left || !right || !out) return QE_ERR_INVALID_ARG;
    const TwoSidedCall q{"qe_result_asof_join", left, right, left_by, right_by, nby, left_out, right_out, nleft_out, nright_out, join_type};
    return guarded(ctx, [&] { *out = run_asof(ctx, q, left_on, right_on, direction, strict); });
}

int32_t qe_ctx_last_asof_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::asof_stats, out); }

}  // extern "C"
