// qe_setop.cpp -- host side of UNION / INTERSECT / EXCEPT [ALL] over two results (kernels: qe_setop.hip): the
// two sides are concatenated with their STRING dictionaries settled (concat_two_sided, qe_exec.h), and every form but UNION ALL
// sorts the concatenation by all its columns and marks the tuple starts (SortedRuns, qe_exec.h), decides per sorted position
// whether its row is kept, and gathers the kept rows with the row gather every operator uses.
#include <algorithm>

#include "qe_exec.h"
#include "qe_kernels.h"
#include "qe_scan.h"

namespace qe {
namespace {

constexpr int kMaxSortedCols = 8, kMaxConcatCols = 16;   // the sort's keys; the limit of qe_result_concat

qe_result *run_set_op(qe_ctx *ctx, const qe_result *left, const qe_result *right, int32_t op, int32_t all) {
    const char *who = "qe_result_set_op";
    if (op < QE_SET_UNION || op > QE_SET_EXCEPT) fail(QE_ERR_INVALID_ARG, std::string(who) + ": unknown op");
    if (all != 0 && all != 1) fail(QE_ERR_INVALID_ARG, std::string(who) + ": all is 0 or 1");
    if (left->cols.size() != right->cols.size()) fail(QE_ERR_INVALID_ARG, std::string(who) + ": the sides differ in their column counts");
    const int32_t ncols = (int32_t)left->cols.size();
    if (ncols == 0) fail(QE_ERR_INVALID_ARG, std::string(who) + ": no column");
    for (int32_t c = 0; c < ncols; c++) {
        const OutColumn &l = left->cols[(size_t)c], &r = right->cols[(size_t)c];
        if (l.type != r.type)
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": column " + std::to_string(c) + " is " + type_name(l.type) + " on the left and " +
                                         type_name(r.type) + " on the right");
        if (l.type == QE_STRING && (!l.dict || !r.dict)) fail(QE_ERR_INVALID_ARG, std::string(who) + ": STRING column without dictionary");
    }
    const bool sorts = !(op == QE_SET_UNION && all);
    if (ncols > (sorts ? kMaxSortedCols : kMaxConcatCols))
        fail(QE_ERR_UNSUPPORTED, std::string(who) + (sorts ? ": more than 8 columns in a form that sorts" : ": more than 16 columns"));
    const int64_t nl = left->count, nr = right->count, n = nl + nr;
    if (n > kMaxRows) fail(QE_ERR_UNSUPPORTED, std::string(who) + ": 2^32 - 1 rows or more");
    need_device(ctx);

    // ---- 1. the concatenated source with its dictionaries settled: left rows, then right rows ----
    PoolScratch sc(ctx);
    TwoSided both = concat_two_sided(ctx, sc, left, 0, right, nl);
    ResultPtr &cat = both.cat;
    int64_t stats[4] = {nl, nr, 0, (int64_t)__builtin_popcount(both.translated)};
    if (!sorts || n == 0) {   // UNION ALL is the concatenation; of no rows at all every form is
        QE_HIP(hipStreamSynchronize(ctx->stream));
        ctx->set_stats.store(stats);
        return cat.release();
    }

    // ---- 2. the sort by every column, and the tuple starts through the same row ids ----
    std::vector<qe_sort_key> keys;
    for (int32_t c = 0; c < ncols; c++) keys.push_back({c, 0});
    SortedRuns runs(ctx, sc, cat.get(), keys.data(), ncols);
    const uint32_t *perm = runs.rows;
    const int64_t nwords = bitmap_words(n);
    unsigned long long *pstart = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    unsigned long long *peer = (unsigned long long *)sc.alloc(bitmap_bytes(n));   // equals pstart: every key is a partition key
    unsigned long long *d_count = (unsigned long long *)sc.alloc(16);
    uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(nwords + 1) * 4);
    uint32_t *pstart_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
    runs.flag(ncols, pstart, peer, d_count);
    runs.rank_starts(pstart, pstart_prefix, sums);
    unsigned long long h_count = 0;
    QE_HIP(hipMemcpyAsync(&h_count, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));   // G: joins the sort's own read-backs
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t G = checked_runs(who, h_count, "tuples", n);
    stats[2] = G;

    // ---- 3. the kept rows ----
    const unsigned long long *keep = pstart;   // UNION: one row per tuple, its first
    const uint32_t *keep_prefix = pstart_prefix;
    int64_t nout = G;
    if (op != QE_SET_UNION) {
        uint32_t *gstart = (uint32_t *)sc.alloc((size_t)(G + 1) * 4);
        unsigned long long *side = (unsigned long long *)sc.alloc(bitmap_bytes(n));
        uint32_t *side_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
        unsigned long long *kept = (unsigned long long *)sc.alloc(bitmap_bytes(n));
        uint32_t *kept_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
        bitmap_positions(ctx->stream, (const uint64_t *)pstart, nullptr, n, pstart_prefix, gstart, G + 1, true);
        // The sort is stable and started from the identity, and the left rows are rows 0 .. nl - 1 of the concatenation: inside
        // one tuple the left rows (perm[j] < nl) stand first, each side in input order.  "The first k rows of a tuple" below
        // relies on this, and so does cL = side bits of the tuple's range.
        launch_setop_side_bits(ctx->stream, perm, n, nl, side);
        bitmap_ranks(ctx->stream, (const uint64_t *)side, nullptr, n, side_prefix, sums, nullptr);
        SetopKeepArgs ka{};
        ka.op = op;
        ka.all = all;
        ka.n = n;
        ka.ntuples = G;
        ka.pstart = pstart;
        ka.side = side;
        ka.pstart_prefix = pstart_prefix;
        ka.side_prefix = side_prefix;
        ka.gstart = gstart;
        ka.keep = kept;
        launch_setop_keep(ctx->stream, ka);
        bitmap_ranks(ctx->stream, (const uint64_t *)kept, nullptr, n, kept_prefix, sums, d_count);
        unsigned long long h_kept = 0;
        QE_HIP(hipMemcpyAsync(&h_kept, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));   // the one read-back besides the sort's and G
        QE_HIP(hipGetLastError());
        QE_HIP(hipStreamSynchronize(ctx->stream));
        nout = (int64_t)h_kept;
        if (nout < 0 || nout > n) fail(QE_ERR_INTERNAL, std::string(who) + ": kept " + std::to_string(nout) + " of " + std::to_string(n) + " rows");
        keep = kept;
        keep_prefix = kept_prefix;
    }

    // ---- 4. kept sorted positions -> source rows -> the output ----
    ResultPtr res = new_result(ctx, nout);
    res->cols.reserve((size_t)ncols);
    for (const OutColumn &c : cat->cols) add_column(ctx, res.get(), c.type, c.nullable, c.dict, nout);
    if (nout > 0) {
        uint32_t *pos = (uint32_t *)sc.alloc((size_t)nout * 4), *rows = (uint32_t *)sc.alloc((size_t)nout * 4);
        bitmap_positions(ctx->stream, (const uint64_t *)keep, nullptr, n, keep_prefix, pos, nout, false);
        launch_gather_rows(ctx->stream, 4, perm, pos, nout, rows);
        gather_columns(ctx, cat->cols, rows, nout, res.get());
    }
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));   // the concatenation and the scratch go back to the pool now
    ctx->set_stats.store(stats);
    return res.release();
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int32_t qe_result_set_op(qe_ctx *ctx, const qe_result *left, const qe_result *right, int32_t op, int32_t all, qe_result **out) {
    if (out) *out = nullptr;
    if (!ctx || !left || !right || !out) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] { *out = run_set_op(ctx, left, right, op, all); });
}

int32_t qe_ctx_last_set_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::set_stats, out); }

}  // extern "C"
