// qe_ordered.cpp -- host side of the ordered-set aggregates per group (kernels: qe_ordered.hip): one sort by
// (group columns, argument) with its boundary flags (SortedRuns, qe_exec.h) per distinct argument column, then word ranks,
// compacted group and run starts, the first valid row of every group, and one small pass per function.  Output columns that hold source values are the existing row gather over a per-group source-row list.
#include <algorithm>
#include <cmath>

#include "qe_exec.h"
#include "qe_kernels.h"
#include "qe_scan.h"

namespace qe {
namespace {

constexpr int kMaxGroupCols = 7, kMaxOrderedFns = 16;   // group columns + one argument = the sort's 8 keys

bool is_percentile(int fn) { return fn == QE_OSA_PERCENTILE_CONT || fn == QE_OSA_PERCENTILE_DISC; }

qe_result *run_group_ordered(qe_ctx *ctx, const qe_result *src, const int32_t *group_cols, int32_t ngroup, const qe_ordered_agg *fns, int32_t nfn) {
    const char *who = "qe_result_group_ordered";
    const int32_t ncols = (int32_t)src->cols.size();
    if (ngroup < 0 || ngroup > kMaxGroupCols) fail(QE_ERR_INVALID_ARG, std::string(who) + ": 0 <= ngroup <= 7");
    if (nfn < 0 || nfn > kMaxOrderedFns) fail(QE_ERR_INVALID_ARG, std::string(who) + ": 0 <= nfn <= 16");
    if (ngroup + nfn < 1) fail(QE_ERR_INVALID_ARG, std::string(who) + ": no group column and no function");
    if ((ngroup > 0 && !group_cols) || (nfn > 0 && !fns)) fail(QE_ERR_INVALID_ARG, std::string(who) + ": null list");
    auto check_column = [&](int32_t c, const char *what) {
        if (c < 0 || c >= ncols) fail(QE_ERR_INVALID_ARG, std::string(who) + ": " + what + " column out of range");
        if (src->cols[(size_t)c].type == QE_STRING && !src->cols[(size_t)c].dict)
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": STRING " + what + " column without dictionary");
    };
    for (int32_t k = 0; k < ngroup; k++) check_column(group_cols[k], "group");
    std::vector<int32_t> args;   // the distinct argument columns, in order of first use: one sort each
    for (int32_t f = 0; f < nfn; f++) {
        const qe_ordered_agg &w = fns[f];
        if (w.fn < QE_OSA_COUNT_DISTINCT || w.fn > QE_OSA_MODE) fail(QE_ERR_INVALID_ARG, std::string(who) + ": unknown function");
        check_column(w.column, "argument");
        const int t = src->cols[(size_t)w.column].type;
        if (w.fn == QE_OSA_PERCENTILE_CONT && (t == QE_BOOLEAN || t == QE_STRING))
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": PERCENTILE_CONT over a " + type_name(t) + " column");
        if (is_percentile(w.fn) && !(w.fraction >= 0.0 && w.fraction <= 1.0))
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": a percentile's fraction lies in [0, 1]");
        if (std::find(args.begin(), args.end(), w.column) == args.end()) args.push_back(w.column);
    }
    const int64_t n = src->count;
    if (n >= (1ll << 32)) fail(QE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 rows");
    need_device(ctx);

    // the output schema: group columns, then one column per function
    auto add_schema = [&](qe_result *res, int64_t rows) {
        res->cols.reserve((size_t)(ngroup + nfn));
        for (int32_t k = 0; k < ngroup; k++) {
            const OutColumn &c = src->cols[(size_t)group_cols[k]];
            add_column(ctx, res, c.type, c.validity != nullptr, c.dict, rows);
        }
        for (int32_t f = 0; f < nfn; f++) {
            const OutColumn &c = src->cols[(size_t)fns[f].column];
            if (fns[f].fn == QE_OSA_COUNT_DISTINCT) add_column(ctx, res, QE_DOUBLE, false, nullptr, rows);
            else if (fns[f].fn == QE_OSA_PERCENTILE_CONT) add_column(ctx, res, QE_DOUBLE, true, nullptr, rows);
            else add_column(ctx, res, c.type, true, c.dict, rows);
        }
    };
    int64_t stats[4] = {n, 0, 0, 0};
    if (n == 0) {   // no group at all, or (no group columns) the one group of nothing: COUNT_DISTINCT 0, everything else NULL
        const int64_t rows = ngroup == 0 ? 1 : 0;
        ResultPtr res = new_result(ctx, rows);
        add_schema(res.get(), rows);
        if (rows) {
            for (OutColumn &c : res->cols) {
                QE_HIP(hipMemsetAsync(c.data, 0, column_bytes(c.type, rows), ctx->stream));
                if (c.validity) QE_HIP(hipMemsetAsync(c.validity, 0, bitmap_bytes(rows), ctx->stream));
            }
            QE_HIP(hipStreamSynchronize(ctx->stream));
        }
        stats[1] = rows;
        ctx->ordered_stats.store(stats);
        return res.release();
    }

    PoolScratch sc(ctx);
    const int64_t nwords = bitmap_words(n);
    unsigned long long *pstart = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    unsigned long long *peer = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    unsigned long long *d_ngroups = (unsigned long long *)sc.alloc(16);
    uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(nwords + 1) * 4);
    uint32_t *pstart_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
    ResultPtr res = own_result(ctx, nullptr);
    int64_t G = 0;
    uint32_t *gstart = nullptr, *first = nullptr, *rows = nullptr;   // sized by G, after the first flags pass

    const size_t nsorts = args.empty() ? 1 : args.size();
    for (size_t s_ = 0; s_ < nsorts; s_++) {
        const int32_t arg = args.empty() ? -1 : args[s_];
        // ---- the sort by (group columns, argument) and the boundary flags through the same row ids ----
        PoolScratch ss(ctx);
        std::vector<qe_sort_key> keys;
        for (int32_t k = 0; k < ngroup; k++) keys.push_back({group_cols[k], 0});
        if (arg >= 0) keys.push_back({arg, 0});
        SortedRuns runs(ctx, ss, src, keys.data(), (int32_t)keys.size());
        const uint32_t *perm = runs.rows;
        runs.flag(ngroup, pstart, peer, d_ngroups);
        // The groups of this sort: the count sizes the output (first sort) and must be the same in every sort.  The read-back
        // joins those the sort itself makes per key (SortDriver::varying).
        unsigned long long h_ngroups = 0;
        QE_HIP(hipMemcpyAsync(&h_ngroups, d_ngroups, 8, hipMemcpyDeviceToHost, ctx->stream));
        QE_HIP(hipGetLastError());
        QE_HIP(hipStreamSynchronize(ctx->stream));
        if (s_ == 0) {
            G = checked_runs(who, h_ngroups, "groups", n);
            res = new_result(ctx, G);
            add_schema(res.get(), G);
            gstart = (uint32_t *)sc.alloc((size_t)(G + 1) * 4);
            first = (uint32_t *)sc.alloc((size_t)G * 4);
            rows = (uint32_t *)sc.alloc((size_t)G * 4);
        } else if ((int64_t)h_ngroups != G) {
            fail(QE_ERR_INTERNAL, std::string(who) + ": the sort on column " + std::to_string(arg) + " found " + std::to_string(h_ngroups) +
                                      " groups, the first sort " + std::to_string(G));
        }
        stats[2]++;
        stats[3] += runs.radix_passes();

        // ---- group starts; the key columns come from the first sort ----
        runs.rank_starts(pstart, pstart_prefix, sums);
        bitmap_positions(ctx->stream, (const uint64_t *)pstart, nullptr, n, pstart_prefix, gstart, G + 1, true);
        OsaGroups og{};
        og.n = n;
        og.ngroups = G;
        og.perm = perm;
        og.gstart = gstart;
        og.first = first;
        if (s_ == 0 && ngroup > 0) {
            launch_osa_rows(ctx->stream, og, QE_OSA_ROWS_KEY, 0.0, nullptr, rows);
            for (int32_t k = 0; k < ngroup; k++) {
                const OutColumn &c = src->cols[(size_t)group_cols[k]];
                gather_column(ctx, c.type, c.data, c.validity, rows, G, res->cols[(size_t)k], kGatherBlocks);
            }
        }
        if (arg < 0) break;   // SELECT DISTINCT: the key tuples are the result

        // ---- the argument: validity in sorted order, first valid row of every group ----
        const OutColumn &ac = src->cols[(size_t)arg];
        unsigned long long *valid_sorted = nullptr;
        if (ac.validity) {
            valid_sorted = (unsigned long long *)ss.alloc(bitmap_bytes(n));
            launch_gather_bits_rows(ctx->stream, ac.validity, perm, n, (uint64_t *)valid_sorted);
        }
        launch_osa_first_valid(ctx->stream, og, valid_sorted);

        bool need_ranks = false, need_runs = false;
        for (int32_t f = 0; f < nfn; f++) {
            if (fns[f].column != arg) continue;
            need_ranks = need_ranks || fns[f].fn == QE_OSA_COUNT_DISTINCT || fns[f].fn == QE_OSA_MODE;
            need_runs = need_runs || fns[f].fn == QE_OSA_MODE;
        }
        uint32_t *peer_prefix = nullptr;
        unsigned long long *best = nullptr;
        if (need_ranks) {
            peer_prefix = (uint32_t *)ss.alloc((size_t)(nwords + 1) * 4);
            bitmap_ranks(ctx->stream, (const uint64_t *)peer, nullptr, n, peer_prefix, sums, nullptr);
        }
        if (need_runs) {   // every MODE of this argument is the same row list
            uint32_t *runpos = (uint32_t *)ss.alloc((size_t)(n + 1) * 4);
            best = (unsigned long long *)ss.alloc((size_t)G * 8);
            bitmap_positions(ctx->stream, (const uint64_t *)peer, nullptr, n, peer_prefix, runpos, n + 1, true);
            QE_HIP(hipMemsetAsync(best, 0, (size_t)G * 8, ctx->stream));
            launch_osa_mode(ctx->stream, og, runpos, peer_prefix, pstart, pstart_prefix, best);
        }
        for (int32_t f = 0; f < nfn; f++) {
            const qe_ordered_agg &w = fns[f];
            if (w.column != arg) continue;
            OutColumn &oc = res->cols[(size_t)(ngroup + f)];
            if (w.fn == QE_OSA_COUNT_DISTINCT) {
                launch_osa_count_distinct(ctx->stream, og, peer, peer_prefix, (double *)oc.data);
            } else if (w.fn == QE_OSA_PERCENTILE_CONT) {
                launch_osa_percentile_cont(ctx->stream, og, ac.type, ac.data, w.fraction, (double *)oc.data, (unsigned long long *)oc.validity);
            } else {   // a row list, and the gather every operator uses: type, bitmap column, dictionary, zero under NULL
                launch_osa_rows(ctx->stream, og, w.fn == QE_OSA_MODE ? QE_OSA_ROWS_MODE : QE_OSA_ROWS_DISC, w.fraction, best, rows);
                gather_column(ctx, ac.type, ac.data, ac.validity, rows, G, oc, kGatherBlocks);
            }
        }
        // (the sort's scratch goes back to the pool here: everything that reads it is queued on the same stream before
        // whatever takes the buffers next)
    }
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    stats[1] = G;
    ctx->ordered_stats.store(stats);
    return res.release();
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int32_t qe_result_group_ordered(qe_ctx *ctx, const qe_result *result, const int32_t *group_cols, int32_t ngroup, const qe_ordered_agg *fns,
                                int32_t nfn, qe_result **out) {
    if (out) *out = nullptr;
    if (!ctx || !result || !out || (ngroup > 0 && !group_cols) || (nfn > 0 && !fns)) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] { *out = run_group_ordered(ctx, result, group_cols, ngroup, fns, nfn); });
}

int32_t qe_ctx_last_ordered_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::ordered_stats, out); }

}  // extern "C"
