// qe_exec.h -- what the files behind the C ABI share (not part of the ABI, not exported from libqe_hip.so):
//   qe_context.cpp   errors, pools, contexts, dictionaries, batches, expression handles, stream calibrations
//   qe_api.cpp       plan cache + geometry (get_plan), the filter+project executor and its entry points
//   qe_groupby.cpp   the global aggregate and the GROUP BY routes with their entry points
//   qe_result.cpp    results on the device and their way to the host
//   qe_join.cpp      the hash equi-join of two device-resident sides, a result as the next plan's batch
//   qe_window.cpp    window functions over a result: the sort, the boundary flags, the segmented scans
#pragma once

#include <memory>
#include <new>
#include <string>
#include <vector>

#include "qe_internal.h"

namespace qe {
#pragma GCC visibility push(hidden)

// ---- qe_context.cpp ------------------------------------------------------------------------------------
// where a failing call leaves its message: the context's last_error, or (no context yet) the calling thread's slot
std::string &error_slot(qe_ctx *ctx);

template <typename F>
int32_t guarded(qe_ctx *ctx, F &&f) {
    try {
        f();
        return QE_OK;
    } catch (const Error &e) {
        error_slot(ctx) = e.msg;
        return e.code;
    } catch (const std::bad_alloc &) {
        error_slot(ctx) = "host out of memory";
        return QE_ERR_OOM;
    } catch (const std::exception &e) {
        error_slot(ctx) = e.what();
        return QE_ERR_INTERNAL;
    }
}

void need_device(const qe_ctx *ctx);
void free_batch(qe_ctx *ctx, qe_batch *b);

inline size_t type_width(int t) {
    switch (t) {
    case QE_DOUBLE: case QE_INT64: return 8;
    case QE_INT32: case QE_STRING: return 4;
    default: return 0;
    }
}
inline size_t bitmap_bytes(int64_t n) { return (size_t)((n + 63) / 64) * 8; }
inline size_t column_bytes(int t, int64_t n) { return t == QE_BOOLEAN ? bitmap_bytes(n) : type_width(t) * (size_t)n; }

// ---- qe_result.cpp --------------------------------------------------------------------------------------
void free_result(qe_ctx *ctx, qe_result *r);

// ---- qe_api.cpp: plans and launches -------------------------------------------------------------------------
// What get_plan is asked for; a call site names only what it sets.
struct PlanRequest {
    const qe_expr *filter = nullptr;
    const qe_expr *const *projs = nullptr;   // projections, or (agg_fns set) the aggregates' inputs
    int32_t nproj = 0;
    const int32_t *agg_fns = nullptr;        // one QE_AGG_* per projection: aggregate mode
    const qe_expr *const *keys = nullptr;    // GROUP BY keys (aggregate mode)
    int32_t nkeys = 0;
    int geo_cand = 0;                        // geometry candidate (qe_ctx::GeoChoice): 0 default, 1 wide, 2 mid
    bool dense = false;                      // filter+project: the dense single-pass kernel
    const std::vector<int> *conj_order = nullptr;   // measured evaluation order of the filter's conjuncts
    int hp_parts = 0, hp_shift = 0;          // hashed GROUP BY: the hash-partitioned form, partitions and 2^shift buckets each
    bool load = true;                        // false: compile (or hit the cache) only, no module is loaded -- needs no device
};
std::shared_ptr<Plan> get_plan(qe_ctx *ctx, const qe_batch *batch, const PlanRequest &rq);

int device_cus(int device);
void fill_inputs(FusedParams &p, const qe_batch *batch, const Plan &plan);
void launch_fused(qe_ctx *ctx, const Plan &plan, FusedParams &p, int grid, bool timed = false);
void collect_time(qe_ctx *ctx);

// ---- qe_groupby.cpp ------------------------------------------------------------------------------------------
struct AggregateCall {
    qe_ctx *ctx;
    const qe_batch *batch;
    const qe_expr *filter;
    const qe_expr *const *keys;    // null: global aggregate
    int32_t nkeys;
    const qe_expr *const *exprs;
    const int32_t *agg_fns;
    int32_t nagg;
    PlanRequest request(bool load = true) const {
        PlanRequest rq{filter, exprs, nagg, agg_fns, keys, nkeys};
        rq.load = load;
        return rq;
    }
};
void run_global_aggregate(const AggregateCall &q, double *out_values, uint8_t *out_valid, int64_t *out_selected_rows);
// GROUP BY: picks the route (dense table, hashed, dense ids, hash-partitioned), sets ctx->last_form
qe_result *run_groupby(const AggregateCall &q);

#pragma GCC visibility pop
}  // namespace qe
