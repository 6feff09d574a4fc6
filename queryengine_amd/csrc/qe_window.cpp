// qe_window.cpp -- host side of the window operator (kernels: qe_window.hip): sort by (partition columns,
// order keys) and mark partition and peer starts (SortedRuns, qe_exec.h), gather every column, then one segmented scan per
// function over the gathered columns.  A frame other than the running one is two scans kept as {value, count} pairs -- shared
// by every function of the call that needs the same ones -- and one elementwise combine per function.
#include <algorithm>

#include "qe_exec.h"
#include "qe_kernels.h"

namespace qe {
namespace {

constexpr int kMaxWindowKeys = 8, kMaxWindowFns = 16;

bool is_rank_fn(int fn) { return fn == QE_WIN_ROW_NUMBER || fn == QE_WIN_RANK || fn == QE_WIN_DENSE_RANK; }
bool is_numeric_agg(int fn) { return fn == QE_WIN_SUM || fn == QE_WIN_MIN || fn == QE_WIN_MAX || fn == QE_WIN_AVG; }
bool is_shift_fn(int fn) { return fn == QE_WIN_LAG || fn == QE_WIN_LEAD; }
bool is_value_fn(int fn) { return fn == QE_WIN_FIRST_VALUE || fn == QE_WIN_LAST_VALUE; }
bool is_aggregate(int fn) { return fn >= QE_WIN_SUM && fn <= QE_WIN_AVG; }
// the frame qe_result_window has always had: the scan's own result is the value, no combine pass
bool is_running(const qe_window_frame_fn &w) { return w.preceding == QE_FRAME_UNBOUNDED && w.following == 0; }

// max_fn: the last function the entry point knows (qe_result_window stops at QE_WIN_LEAD)
qe_result *run_window(qe_ctx *ctx, const char *who, int max_fn, const qe_result *src, const int32_t *part, int32_t npart, const qe_sort_key *order,
                      int32_t norder, const qe_window_frame_fn *fns, int32_t nfn) {
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
        const qe_window_frame_fn &w = fns[f];
        if (w.fn < QE_WIN_ROW_NUMBER || w.fn > max_fn) fail(QE_ERR_INVALID_ARG, std::string(who) + ": unknown window function");
        if (w.preceding < QE_FRAME_UNBOUNDED || w.preceding >= (1ll << 31) || w.following < QE_FRAME_UNBOUNDED || w.following >= (1ll << 31))
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": preceding and following are QE_FRAME_UNBOUNDED or in [0, 2^31)");
        if ((is_rank_fn(w.fn) || is_shift_fn(w.fn)) && (w.preceding != 0 || w.following != 0))
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": the ranks and LAG / LEAD take no frame (preceding = following = 0)");
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
        const qe_window_frame_fn &w = fns[f];
        if (is_rank_fn(w.fn)) add_column(ctx, res.get(), QE_INT64, false, nullptr, n);
        else if (is_value_fn(w.fn))
            add_column(ctx, res.get(), src->cols[(size_t)w.column].type, src->cols[(size_t)w.column].validity != nullptr, src->cols[(size_t)w.column].dict, n);
        else if (is_shift_fn(w.fn)) add_column(ctx, res.get(), src->cols[(size_t)w.column].type, true, src->cols[(size_t)w.column].dict, n);
        else add_column(ctx, res.get(), QE_DOUBLE, w.fn != QE_WIN_COUNT, nullptr, n);
    }
    const int64_t ntiles = (n + kWinTileRows - 1) / kWinTileRows;
    int64_t stats[4] = {n, 0, ntiles, n > 0 ? (ntiles + kWinTripTiles - 1) / kWinTripTiles : 0};
    if (n == 0) {
        ctx->window_stats.store(stats);
        return res.release();
    }

    PoolScratch sc(ctx);
    unsigned long long *pstart = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    unsigned long long *peer = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    unsigned long long *d_nparts = (unsigned long long *)sc.alloc(16);
    unsigned long long h_nparts = 0;
    {
        // ---- sort + gather (skipped without keys: the columns are copied), then the boundary flags through the same row ids ----
        PoolScratch ss(ctx);
        SortedRuns runs(ctx, ss, src, keys.data(), (int32_t)keys.size());
        if (runs.rows) {
            gather_columns(ctx, src->cols, runs.rows, n, res.get());
        } else {
            for (size_t c = 0; c < src->cols.size(); c++) {
                const OutColumn &s_ = src->cols[c];
                QE_HIP(hipMemcpyAsync(res->cols[c].data, s_.data, column_bytes(s_.type, n), hipMemcpyDeviceToDevice, ctx->stream));
                if (s_.validity) QE_HIP(hipMemcpyAsync(res->cols[c].validity, s_.validity, bitmap_bytes(n), hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        runs.flag(npart, pstart, peer, d_nparts);
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
    bool need_start = false, need_first_peer = false, need_end = false;
    for (int32_t f = 0; f < nfn; f++) {
        const bool framed = is_value_fn(fns[f].fn) || (is_aggregate(fns[f].fn) && !is_running(fns[f]));
        need_start = need_start || fns[f].fn == QE_WIN_ROW_NUMBER || fns[f].fn == QE_WIN_RANK || is_shift_fn(fns[f].fn) || framed;
        need_first_peer = need_first_peer || fns[f].fn == QE_WIN_RANK;
        need_end = need_end || framed;
    }
    const uint32_t *start = need_start ? index_of(pstart) : nullptr;
    const uint32_t *first_peer = need_first_peer ? index_of(peer) : nullptr;
    const uint32_t *end = nullptr;   // index of the partition's last row: the mirror of `start`, one reverse scan
    if (need_end) {
        uint32_t *idx = (uint32_t *)sc.alloc((size_t)n * 4);
        WinScanArgs a = base;
        a.op = QE_WSCAN_INDEX;
        a.out_mode = QE_WOUT_INDEX;
        a.reverse = 1;
        a.validity = pstart;
        a.out = idx;
        launch_win_scan(ctx->stream, a);
        end = idx;
    }

    // the argument of an aggregate as a scan reads it
    auto scan_of = [&](const qe_window_frame_fn &w) {
        WinScanArgs a = base;
        a.pstart = pstart;
        const OutColumn &arg = res->cols[(size_t)w.column];   // the gathered column
        a.validity = (const unsigned long long *)arg.validity;
        a.type = arg.type;
        a.data = w.fn == QE_WIN_COUNT ? nullptr : arg.data;
        a.op = w.fn == QE_WIN_MIN ? QE_WSCAN_MIN : w.fn == QE_WIN_MAX ? QE_WSCAN_MAX : QE_WSCAN_SUM;
        a.out_mode = w.fn == QE_WIN_SUM ? QE_WOUT_SUM : w.fn == QE_WIN_AVG ? QE_WOUT_AVG : w.fn == QE_WIN_COUNT ? QE_WOUT_COUNT : QE_WOUT_MINMAX;
        return a;
    };
    // The scanned pairs of (column, combination, direction, block), made once per call: SUM, AVG and COUNT of one column over
    // one frame read the same two scans.  A COUNT's scan reads no values unless a SUM / AVG of the call wants the same column.
    struct PairScan {
        int32_t column;
        int op, reverse;
        int64_t block;
        double *v;
        uint32_t *c;
    };
    std::vector<PairScan> pairs;
    auto pair_scan = [&](const qe_window_frame_fn &w, int reverse, int64_t block) {
        WinScanArgs a = scan_of(w);
        for (const PairScan &p : pairs)
            if (p.column == w.column && p.op == a.op && p.reverse == reverse && p.block == block) return p;
        if (a.op == QE_WSCAN_SUM) {
            a.data = nullptr;
            for (int32_t g = 0; g < nfn; g++)
                if ((fns[g].fn == QE_WIN_SUM || fns[g].fn == QE_WIN_AVG) && fns[g].column == w.column) a.data = res->cols[(size_t)w.column].data;
        }
        PairScan p{w.column, a.op, reverse, block, (double *)sc.alloc((size_t)n * 8), (uint32_t *)sc.alloc((size_t)n * 4)};
        a.reverse = reverse;
        a.block = block;
        a.out_mode = QE_WOUT_ITEM;
        a.out = p.v;
        a.out_c = p.c;
        a.out_valid = nullptr;
        launch_win_scan(ctx->stream, a);
        pairs.push_back(p);
        return p;
    };

    for (int32_t f = 0; f < nfn; f++) {
        const qe_window_frame_fn &w = fns[f];
        OutColumn &oc = res->cols[(size_t)(ncols + f)];
        if (w.fn == QE_WIN_ROW_NUMBER || w.fn == QE_WIN_RANK) {
            launch_win_rank(ctx->stream, start, w.fn == QE_WIN_RANK ? first_peer : nullptr, n, (int64_t *)oc.data);
        } else if (is_shift_fn(w.fn)) {
            const OutColumn &arg = res->cols[(size_t)w.column];   // the gathered column
            launch_win_shift(ctx->stream, (int)type_width(arg.type), arg.data, arg.validity, start, nullptr, n,
                             w.fn == QE_WIN_LAG ? -w.offset : w.offset, oc.data, oc.validity);
        } else if (is_value_fn(w.fn)) {   // the row at the frame's edge: j - preceding or j + following clamped into the partition
            const OutColumn &arg = res->cols[(size_t)w.column];
            const int64_t reach = w.fn == QE_WIN_FIRST_VALUE ? w.preceding : w.following;
            const int64_t delta = reach == QE_FRAME_UNBOUNDED ? (1ll << 32) : reach;
            launch_win_shift(ctx->stream, (int)type_width(arg.type), arg.data, arg.validity, start, end, n,
                             w.fn == QE_WIN_FIRST_VALUE ? -delta : delta, oc.data, oc.validity);
        } else if (w.fn == QE_WIN_DENSE_RANK) {   // peer groups started in the partition so far
            WinScanArgs a = base;
            a.pstart = pstart;
            a.out = oc.data;
            a.op = QE_WSCAN_SUM;
            a.out_mode = QE_WOUT_COUNT_I64;
            a.validity = peer;
            launch_win_scan(ctx->stream, a);
        } else if (is_running(w)) {
            WinScanArgs a = scan_of(w);
            a.out = oc.data;
            a.out_valid = (unsigned long long *)oc.validity;
            launch_win_scan(ctx->stream, a);
        } else {
            const WinScanArgs proto = scan_of(w);
            const bool bounded = w.preceding >= 0 && w.following >= 0;
            const int64_t block = bounded ? w.preceding + w.following + 1 : 0;
            WinFrameArgs fa{};
            fa.op = proto.op;
            fa.out_mode = proto.out_mode;
            fa.n = n;
            fa.preceding = w.preceding;
            fa.following = w.following;
            fa.start = start;
            fa.end = end;
            if (bounded || w.preceding < 0) {
                const PairScan p = pair_scan(w, 0, block);
                fa.p_v = p.v;
                fa.p_c = p.c;
            }
            if (bounded || w.preceding >= 0) {
                const PairScan p = pair_scan(w, 1, block);
                fa.s_v = p.v;
                fa.s_c = p.c;
            }
            fa.out = oc.data;
            fa.out_valid = (unsigned long long *)oc.validity;
            launch_win_frame(ctx->stream, fa);
        }
    }
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    ctx->window_stats.store(stats);
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
    return guarded(ctx, [&] {   // the same body with the one frame this call has: running for the aggregates
        std::vector<qe_window_frame_fn> framed;
        for (int32_t f = 0; f < nfn && f < kMaxWindowFns + 1; f++) {
            const bool agg = is_aggregate(fns[f].fn);
            framed.push_back({fns[f].fn, fns[f].column, fns[f].offset, agg ? QE_FRAME_UNBOUNDED : 0, 0});
        }
        *out = run_window(ctx, "qe_result_window", QE_WIN_LEAD, result, partition_cols, npart, order, norder, framed.data(), nfn);
    });
}

int32_t qe_result_window_frames(qe_ctx *ctx, const qe_result *result, const int32_t *partition_cols, int32_t npart, const qe_sort_key *order,
                                int32_t norder, const qe_window_frame_fn *fns, int32_t nfn, qe_result **out) {
    if (out) *out = nullptr;
    if (!ctx || !result || !fns || !out) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        *out = run_window(ctx, "qe_result_window_frames", QE_WIN_LAST_VALUE, result, partition_cols, npart, order, norder, fns, nfn);
    });
}

int32_t qe_ctx_last_window_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::window_stats, out); }

}  // extern "C"
