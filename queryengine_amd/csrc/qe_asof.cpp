// qe_asof.cpp -- host side of the ASOF join of two results (kernels: qe_asof.hip): for every left row the one
// right row of the same by tuple whose `on` value is nearest at or before (after) it.  The key columns of the two sides are
// concatenated with their STRING dictionaries settled (concat_two_sided, qe_exec.h), sorted once by (by.., on) and marked
// with the partition starts (SortedRuns, qe_exec.h); two kernels find, per left row, the nearest eligible right position inside its
// partition, and the row gather every operator uses builds the output.
#include <algorithm>

#include "qe_exec.h"
#include "qe_kernels.h"
#include "qe_scan.h"

namespace qe {
namespace {

constexpr int kMaxBy = 7;   // with the `on` column: the sort's 8 keys

struct AsofCall {
    const qe_result *left, *right;
    const int32_t *left_by, *right_by;
    int32_t nby, left_on, right_on, direction, strict, join_type;
    const int32_t *left_out;
    int32_t nleft_out;
    const int32_t *right_out;
    int32_t nright_out;
};

// what can be said without reading either result (a caller's handle is only touched once these hold)
void check_scalars(const AsofCall &q, const char *who) {
    if (q.nby < 0 || q.nby > kMaxBy) fail(QE_ERR_INVALID_ARG, std::string(who) + ": 0 to 7 by columns");
    if (q.nby > 0 && (!q.left_by || !q.right_by)) fail(QE_ERR_INVALID_ARG, std::string(who) + ": by columns missing");
    if (q.direction != QE_ASOF_BACKWARD && q.direction != QE_ASOF_FORWARD) fail(QE_ERR_INVALID_ARG, std::string(who) + ": unknown direction");
    if (q.strict != 0 && q.strict != 1) fail(QE_ERR_INVALID_ARG, std::string(who) + ": strict is 0 or 1");
    if (q.join_type != QE_JOIN_INNER && q.join_type != QE_JOIN_LEFT) fail(QE_ERR_INVALID_ARG, std::string(who) + ": the join type is INNER or LEFT");
    if (q.nleft_out < 0 || q.nright_out < 0) fail(QE_ERR_INVALID_ARG, std::string(who) + ": negative column count");
    if ((q.nleft_out > 0 && !q.left_out) || (q.nright_out > 0 && !q.right_out)) fail(QE_ERR_INVALID_ARG, std::string(who) + ": output columns missing");
    if ((int64_t)q.nleft_out + q.nright_out < 1) fail(QE_ERR_INVALID_ARG, std::string(who) + ": no output column");
}

void check_cols(const qe_result *side, const int32_t *cols, int32_t n, const char *who, const char *what) {
    for (int32_t i = 0; i < n; i++)
        if (cols[i] < 0 || cols[i] >= (int32_t)side->cols.size())
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": " + what + " column " + std::to_string(cols[i]) + " out of range");
}

qe_result *run_asof(qe_ctx *ctx, const AsofCall &q) {
    const char *who = "qe_result_asof_join";
    check_scalars(q, who);
    const qe_result *left = q.left, *right = q.right;
    check_cols(left, q.left_by, q.nby, who, "left by");
    check_cols(right, q.right_by, q.nby, who, "right by");
    check_cols(left, &q.left_on, 1, who, "left on");
    check_cols(right, &q.right_on, 1, who, "right on");
    check_cols(left, q.left_out, q.nleft_out, who, "left output");
    check_cols(right, q.right_out, q.nright_out, who, "right output");
    const int32_t nkeys = q.nby + 1;
    std::vector<int32_t> lkeys(q.left_by, q.left_by + q.nby), rkeys(q.right_by, q.right_by + q.nby);
    lkeys.push_back(q.left_on);
    rkeys.push_back(q.right_on);
    for (int32_t k = 0; k < nkeys; k++) {
        const OutColumn &l = left->cols[(size_t)lkeys[(size_t)k]], &r = right->cols[(size_t)rkeys[(size_t)k]];
        const std::string name = k < q.nby ? "by column " + std::to_string(k) : std::string("the on column");
        if (l.type != r.type)
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": " + name + " is " + type_name(l.type) + " on the left and " + type_name(r.type) + " on the right");
        if (k == q.nby && l.type != QE_DOUBLE && l.type != QE_INT64 && l.type != QE_INT32)
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": the on column is " + type_name(l.type) + ", not DOUBLE, INT64 or INT32");
        if (l.type == QE_STRING && (!l.dict || !r.dict)) fail(QE_ERR_INVALID_ARG, std::string(who) + ": STRING by column without dictionary");
    }
    const int64_t nl = left->count, nr = right->count, n = nl + nr;
    if (n > kMaxRows) fail(QE_ERR_UNSUPPORTED, std::string(who) + ": 2^32 - 1 rows or more");
    need_device(ctx);
    const bool forward = q.direction == QE_ASOF_FORWARD, inner = q.join_type == QE_JOIN_INNER;
    int64_t stats[4] = {nl, nr, 0, 0};

    PoolScratch sc(ctx);
    uint32_t *match = nullptr;            // per left row: its right row or 0xFFFFFFFF
    unsigned long long *matched = nullptr;
    uint32_t *matched_prefix = nullptr, *identity = nullptr;
    int64_t nmatched = 0;
    TwoSided both{own_result(ctx, nullptr)};   // the scratch key result: released with the scratch, after the last kernel
    if (n > 0) {
        // ---- 1. the scratch key result, the dictionaries of its STRING by columns settled.  The stable sort keeps the
        // concatenation's order inside a run of equal keys: the right rows go first where a left row may match an equal `on`
        // looking back, or may not match it looking forward ----
        const qe_result lview = column_view(left, lkeys.data(), nkeys), rview = column_view(right, rkeys.data(), nkeys);
        const bool right_first = forward == (q.strict != 0);
        const int64_t nfirst = right_first ? nr : nl;
        both = concat_two_sided(ctx, sc, &lview, right_first ? nr : 0, &rview, right_first ? 0 : nl);
        const qe_result *cat = both.cat.get();

        // ---- 2. one stable sort over (by.., on), and the partition starts through the same row ids ----
        std::vector<qe_sort_key> keys;
        for (int32_t k = 0; k < nkeys; k++) keys.push_back({k, 0});
        SortedRuns runs(ctx, sc, cat, keys.data(), nkeys);
        const uint32_t *perm = runs.rows;
        const int64_t nwords = bitmap_words(n);
        unsigned long long *pstart = (unsigned long long *)sc.alloc(bitmap_bytes(n));
        unsigned long long *peer = (unsigned long long *)sc.alloc(bitmap_bytes(n));   // the runs of equal `on`: not read
        unsigned long long *eligible = (unsigned long long *)sc.alloc(bitmap_bytes(n));
        unsigned long long *rbits = (unsigned long long *)sc.alloc(bitmap_bytes(n));
        unsigned long long *d_count = (unsigned long long *)sc.alloc(16);   // [0] partitions, [1] matched left rows
        uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(nwords + 1) * 4);
        uint32_t *pstart_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
        uint32_t *right_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
        runs.flag(q.nby, pstart, peer, d_count);
        runs.rank_starts(pstart, pstart_prefix, sums);

        // ---- 3. the rows with a whole key, and the right rows among them ----
        AsofEligibleArgs ea{};
        ea.s = AsofSides{perm, n, nfirst, right_first ? 1 : 0};
        ea.nkeys = nkeys;
        for (int32_t k = 0; k < nkeys; k++) ea.validity[k] = (const unsigned long long *)cat->cols[(size_t)k].validity;
        ea.eligible = eligible;
        ea.right = rbits;
        launch_asof_eligible(ctx->stream, ea);
        bitmap_ranks(ctx->stream, (const uint64_t *)rbits, nullptr, n, right_prefix, sums, nullptr);

        // ---- 4. the pick, and the matches as a bitmap over the left rows ----
        if (nl > 0) {
            uint32_t *rpos = (uint32_t *)sc.alloc((size_t)(nr + 1) * 4);   // the eligible right rows are at most nr; the kernel reads their number
            match = (uint32_t *)sc.alloc((size_t)nl * 4);
            matched = (unsigned long long *)sc.alloc(bitmap_bytes(nl));
            matched_prefix = (uint32_t *)sc.alloc((size_t)(bitmap_words(nl) + 1) * 4);
            if (!inner) identity = (uint32_t *)sc.alloc((size_t)nl * 4);
            bitmap_positions(ctx->stream, (const uint64_t *)rbits, nullptr, n, right_prefix, rpos, nr, false);
            AsofPickArgs pa{};
            pa.s = ea.s;
            pa.forward = forward ? 1 : 0;
            pa.nleft = nl;
            pa.eligible = eligible;
            pa.right = rbits;
            pa.pstart = pstart;
            pa.right_prefix = right_prefix;
            pa.pstart_prefix = pstart_prefix;
            pa.rpos = rpos;
            pa.match = match;
            launch_asof_pick(ctx->stream, pa);
            launch_asof_matched(ctx->stream, match, nl, matched, identity);
            bitmap_ranks(ctx->stream, (const uint64_t *)matched, nullptr, nl, matched_prefix, sums, d_count + 1);
        }
        unsigned long long h_count[2] = {0, 0};
        QE_HIP(hipMemcpyAsync(h_count, d_count, 16, hipMemcpyDeviceToHost, ctx->stream));   // the one read-back besides the sort's own
        QE_HIP(hipGetLastError());
        QE_HIP(hipStreamSynchronize(ctx->stream));
        const int64_t G = checked_runs(who, h_count[0], "partitions", n);
        nmatched = (int64_t)h_count[1];
        if (nmatched < 0 || nmatched > nl) fail(QE_ERR_INTERNAL, std::string(who) + ": matched " + std::to_string(nmatched) + " of " + std::to_string(nl) + " left rows");
        stats[3] = G;
        stats[2] = nmatched;
    }

    // ---- 5. the output: the listed left columns by the kept left rows, the listed right columns by their matches ----
    const int64_t nout = inner ? nmatched : nl;
    ResultPtr res = new_result(ctx, nout);
    res->cols.reserve((size_t)(q.nleft_out + q.nright_out));
    const uint32_t *lrows = identity, *rrows = match;
    if (inner && nout > 0) {
        uint32_t *kept = (uint32_t *)sc.alloc((size_t)nout * 4), *theirs = (uint32_t *)sc.alloc((size_t)nout * 4);
        bitmap_positions(ctx->stream, (const uint64_t *)matched, nullptr, nl, matched_prefix, kept, nout, false);
        launch_gather_rows(ctx->stream, 4, match, kept, nout, theirs);
        lrows = kept;
        rrows = theirs;
    }
    auto emit = [&](const OutColumn &src, const uint32_t *rows, bool force_nullable) {
        OutColumn &oc = add_column(ctx, res.get(), src.type, force_nullable || is_nullable(src), src.dict, nout);
        if (nout > 0) gather_column(ctx, src.type, src.data, src.validity, rows, nout, oc, kGatherBlocks);
    };
    for (int32_t i = 0; i < q.nleft_out; i++) emit(left->cols[(size_t)q.left_out[i]], lrows, false);
    for (int32_t i = 0; i < q.nright_out; i++) emit(right->cols[(size_t)q.right_out[i]], rrows, !inner);
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
    const AsofCall q{left, right, left_by, right_by, nby, left_on, right_on, direction, strict, join_type, left_out, nleft_out, right_out, nright_out};
    return guarded(ctx, [&] { *out = run_asof(ctx, q); });
}

int32_t qe_ctx_last_asof_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::asof_stats, out); }

}  // extern "C"
