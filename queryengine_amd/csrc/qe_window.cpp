// qe_window.cpp -- host side of the window operator (kernels: qe_window.hip): sort by (partition columns,
// order keys) with the ORDER BY driver, gather every column, mark partition and peer starts, then one segmented scan per
// function over the gathered columns.
#include <algorithm>

#include "qe_exec.h"
#include "qe_kernels.h"

namespace qe {
namespace {

constexpr int kMaxWindowKeys = 8, kMaxWindowFns = 16;

bool is_rank_fn(int fn) { return fn == QE_WIN_ROW_NUMBER || fn == QE_WIN_RANK || fn == QE_WIN_DENSE_RANK; }
bool is_numeric_agg(int fn) { return fn == QE_WIN_SUM || fn == QE_WIN_MIN || fn == QE_WIN_MAX || fn == QE_WIN_AVG; }
bool is_shift_fn(int fn) { return fn == QE_WIN_LAG || fn == QE_WIN_LEAD; }

qe_result *run_window(qe_ctx *ctx, const qe_result *src, const int32_t *part, int32_t npart, const qe_sort_key *order, int32_t norder,
                      const qe_window_fn *fns, int32_t nfn) {
    const char *who = "qe_result_window";
    const int32_t ncols = (int32_t)src->cols.size();
    if (npart < 0 || norder < 0 || npart + norder > kMaxWindowKeys) fail(QE_ERR_INVALID_ARG, std::string(who) + ": 0 <= npart + norder <= 8");
    if ((npart > 0 && !part) || (norder > 0 && !order)) fail(QE_ERR_INVALID_ARG, std::string(who) + ": null key list");
    if (nfn < 1 || nfn > kMaxWindowFns) fail(QE_ERR_INVALID_ARG, std::string(who) + ": 1 <= nfn <= 16");
    std::vector<qe_sort_key> keys;
    for (int32_t k = 0; k < npart; k++) keys.push_back({part[k], 0});
    for (int32_t k = 0; k < norder; k++) keys.push_back(order[k]);
    for (const qe_sort_key &k : keys) {
        if (k.column < 0 || k.column >= ncols) fail(QE_ERR_INVALID_ARG, std::string(who) + ": key column out of range");
        if (src->cols[(size_t)k.column].type == QE_STRING && !src->cols[(size_t)k.column].dict)
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": STRING key without dictionary");
    }
    for (int32_t f = 0; f < nfn; f++) {
        const qe_window_fn &w = fns[f];
        if (w.fn < QE_WIN_ROW_NUMBER || w.fn > QE_WIN_LEAD) fail(QE_ERR_INVALID_ARG, std::string(who) + ": unknown window function");
        if (is_rank_fn(w.fn)) continue;
        if (w.column < 0 || w.column >= ncols) fail(QE_ERR_INVALID_ARG, std::string(who) + ": argument column out of range");
        const int t = src->cols[(size_t)w.column].type;
        if (is_numeric_agg(w.fn) && (t == QE_BOOLEAN || t == QE_STRING))
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": SUM / MIN / MAX / AVG over a " + type_name(t) + " column");
        if (is_shift_fn(w.fn) && (w.offset < 0 || w.offset >= (1ll << 31))) fail(QE_ERR_INVALID_ARG, std::string(who) + ": 0 <= offset < 2^31");
    }
    const int64_t n = src->count;
    if (n >= (1ll << 32)) fail(QE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 rows");
    need_device(ctx);

    ResultPtr res = new_result(ctx, n);
    res->cols.reserve((size_t)(ncols + nfn));
    for (const OutColumn &c : src->cols) add_column(ctx, res.get(), c.type, c.validity != nullptr, c.dict, n);
    for (int32_t f = 0; f < nfn; f++) {
        const qe_window_fn &w = fns[f];
        if (is_rank_fn(w.fn)) add_column(ctx, res.get(), QE_INT64, false, nullptr, n);
        else if (is_shift_fn(w.fn)) add_column(ctx, res.get(), src->cols[(size_t)w.column].type, true, src->cols[(size_t)w.column].dict, n);
        else add_column(ctx, res.get(), QE_DOUBLE, w.fn != QE_WIN_COUNT, nullptr, n);
    }
    const int64_t ntiles = (n + kWinTileRows - 1) / kWinTileRows;
    int64_t stats[4] = {n, 0, ntiles, n > 0 ? (ntiles + kWinTripTiles - 1) / kWinTripTiles : 0};
    if (n == 0) {
        for (int i = 0; i < 4; i++) ctx->window_stats[i] = stats[i];
        return res.release();
    }

    PoolScratch sc(ctx);
    unsigned long long *pstart = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    unsigned long long *peer = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    unsigned long long *d_nparts = (unsigned long long *)sc.alloc(16);
    QE_HIP(hipMemsetAsync(d_nparts, 0, 16, ctx->stream));
    unsigned long long h_nparts = 0;
    {
        // ---- sort + gather (skipped without keys: the columns are copied), then the boundary flags through the same row ids ----
        PoolScratch ss(ctx);
        const int32_t nkeys = (int32_t)keys.size();
        SortDriver drv{ctx, ss, src, keys.data(), nkeys};
        WinFlagArgs fa{};
        fa.nkeys = nkeys;
        fa.npart = npart;
        fa.n = n;
        fa.pstart = pstart;
        fa.peer = peer;
        fa.npartitions = d_nparts;
        if (nkeys > 0) {
            drv.prepare();
            RadixBuffers rb(ss, n);
            drv.sort(rb, true);
            gather_columns(ctx, src->cols, rb.sorted_rows(), n, res.get());
            fa.perm = rb.sorted_rows();
            for (int32_t k = 0; k < nkeys; k++) {
                const OutColumn &kc = src->cols[(size_t)keys[(size_t)k].column];
                fa.type[k] = kc.type;
                fa.data[k] = kc.data;
                fa.validity[k] = (const unsigned long long *)kc.validity;
                fa.ranks[k] = drv.d_ranks[(size_t)k];
                fa.nranks[k] = drv.nranks[(size_t)k];
            }
        } else {
            for (size_t c = 0; c < src->cols.size(); c++) {
                const OutColumn &s_ = src->cols[c];
                QE_HIP(hipMemcpyAsync(res->cols[c].data, s_.data, column_bytes(s_.type, n), hipMemcpyDeviceToDevice, ctx->stream));
                if (s_.validity) QE_HIP(hipMemcpyAsync(res->cols[c].validity, s_.validity, bitmap_bytes(n), hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        launch_win_flags(ctx->stream, fa);
        QE_HIP(hipMemcpyAsync(&h_nparts, d_nparts, 8, hipMemcpyDeviceToHost, ctx->stream));
        QE_HIP(hipGetLastError());
        QE_HIP(hipStreamSynchronize(ctx->stream));   // the sort's scratch goes back to the pool here
    }
    stats[1] = (int64_t)h_nparts;

    // ---- the scans ----
    WinScanArgs base{};
    base.n = n;
    base.ntiles = ntiles;
    base.tile_v = (double *)sc.alloc((size_t)ntiles * 8);
    base.carry_v = (double *)sc.alloc((size_t)ntiles * 8);
    base.tile_c = (unsigned int *)sc.alloc((size_t)ntiles * 4);
    base.tile_f = (unsigned int *)sc.alloc((size_t)ntiles * 4);
    base.carry_c = (unsigned int *)sc.alloc((size_t)ntiles * 4);
    // index of the last set bit of `bits` at or before every row: the partition start, the first peer
    auto index_of = [&](const unsigned long long *bits) {
        uint32_t *idx = (uint32_t *)sc.alloc((size_t)n * 4);
        WinScanArgs a = base;
        a.op = QE_WSCAN_INDEX;
        a.out_mode = QE_WOUT_INDEX;
        a.validity = bits;
        a.out = idx;
        launch_win_scan(ctx->stream, a);
        return idx;
    };
    bool need_start = false, need_first_peer = false;
    for (int32_t f = 0; f < nfn; f++) {
        need_start = need_start || fns[f].fn == QE_WIN_ROW_NUMBER || fns[f].fn == QE_WIN_RANK || is_shift_fn(fns[f].fn);
        need_first_peer = need_first_peer || fns[f].fn == QE_WIN_RANK;
    }
    const uint32_t *start = need_start ? index_of(pstart) : nullptr;
    const uint32_t *first_peer = need_first_peer ? index_of(peer) : nullptr;

    for (int32_t f = 0; f < nfn; f++) {
        const qe_window_fn &w = fns[f];
        OutColumn &oc = res->cols[(size_t)(ncols + f)];
        if (w.fn == QE_WIN_ROW_NUMBER || w.fn == QE_WIN_RANK) {
            launch_win_rank(ctx->stream, start, w.fn == QE_WIN_RANK ? first_peer : nullptr, n, (int64_t *)oc.data);
        } else if (is_shift_fn(w.fn)) {
            const OutColumn &arg = res->cols[(size_t)w.column];   // the gathered column
            launch_win_shift(ctx->stream, (int)type_width(arg.type), arg.data, arg.validity, start, n, w.fn == QE_WIN_LAG ? -w.offset : w.offset,
                             oc.data, oc.validity);
        } else {
            WinScanArgs a = base;
            a.pstart = pstart;
            a.out = oc.data;
            a.out_valid = (unsigned long long *)oc.validity;
            if (w.fn == QE_WIN_DENSE_RANK) {   // peer groups started in the partition so far
                a.op = QE_WSCAN_SUM;
                a.out_mode = QE_WOUT_COUNT_I64;
                a.validity = peer;
            } else {
                const OutColumn &arg = res->cols[(size_t)w.column];
                a.validity = (const unsigned long long *)arg.validity;
                a.type = arg.type;
                a.data = w.fn == QE_WIN_COUNT ? nullptr : arg.data;
                a.op = w.fn == QE_WIN_MIN ? QE_WSCAN_MIN : w.fn == QE_WIN_MAX ? QE_WSCAN_MAX : QE_WSCAN_SUM;
                a.out_mode = w.fn == QE_WIN_SUM ? QE_WOUT_SUM : w.fn == QE_WIN_AVG ? QE_WOUT_AVG : w.fn == QE_WIN_COUNT ? QE_WOUT_COUNT : QE_WOUT_MINMAX;
            }
            launch_win_scan(ctx->stream, a);
        }
    }
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 4; i++) ctx->window_stats[i] = stats[i];
    return res.release();
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int32_t qe_result_window(qe_ctx *ctx, const qe_result *result, const int32_t *partition_cols, int32_t npart, const qe_sort_key *order,
                         int32_t norder, const qe_window_fn *fns, int32_t nfn, qe_result **out) {
    if (out) *out = nullptr;
    if (!ctx || !result || !fns || !out) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] { *out = run_window(ctx, result, partition_cols, npart, order, norder, fns, nfn); });
}

int32_t qe_ctx_last_window_stats(const qe_ctx *ctx, int64_t out[4]) {
    if (!ctx || !out) return QE_ERR_INVALID_ARG;
    for (int i = 0; i < 4; i++) out[i] = ctx->window_stats[i];
    return QE_OK;
}

}  // extern "C"
