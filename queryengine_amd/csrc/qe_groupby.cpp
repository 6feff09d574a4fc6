// qe_groupby.cpp -- the aggregating executors behind the C ABI: the global aggregate (qe_filter_aggregate) and GROUP BY
// (qe_filter_groupby): run_groupby picks the route -- dense table, hashed table, dense ids or hash partitions.
// What an accumulator's words mean and how a group becomes a result row is qe_group_finish.h's; this file launches and uploads.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "qe_exec.h"
#include "qe_group_finish.h"
#include "qe_kernels.h"
#include "qe_scan.h"

using namespace qe;

namespace {

constexpr int kScatterWgsPerCu = 2;   // workgroups per CU of the partitioned group-by's scatter pass

// Environment knobs of the routes (measurement switches, not API), read once per process.
struct Knobs {
    // hashed form: more keys than this and the next executions of the plan resolve dense ids first (300 keys: 15 ms probing the
    // LDS tables, 6.6 ms as build pass + dense LDS group-by; crossover ~70 keys)
    int64_t ids_from = env("QE_IDS_FROM", 64);
    // hash-partitioned form: results of this many groups are finished on the device (1 M groups cost the host ~70 ms)
    int64_t groups_on_device_from = env("QE_GROUPS_ON_DEVICE_FROM", 4096);
    // key-range form, scatter pass: two workgroups per CU -- the 64 KiB LDS stage of the tile sort lets two share a CU (one sorts
    // and stores while the other waits for its loads)
    int scatter_wgs_per_cu = (int)env("QE_GB_SCATTER_WGS_PER_CU", kScatterWgsPerCu);
    // key-range form, aggregate pass: ~512 workgroups, one LDS table each, merged into the global table
    int agg_wgs = (int)env("QE_GB_AGG_WGS", 512);
    // keys (known from an earlier execution) from which the hash-partitioned form replaces id build + dense passes.  Measured,
    // SELECT k, MIN(v), MAX(v) over 1 B rows, ids against this form: 30 000 keys 21 / 14.7 ms, 100 000 keys 24.0 / 15.3, 300 000
    // keys 32.1 / 17.8, 1 000 000 keys 57 / 24.4; below 25 000 keys, this form / ids: 20 000 keys 14.9 / 20.2, 10 000 keys 15.9 /
    // 16.9, 5000 keys 16.3 / 16.8, 3000 keys 17.2 / 18.3 (fewer fit the LDS-privatised table)
    int64_t hp_from = env("QE_HP_FROM", 4000);
    int hp_parts = (int)env("QE_HP_PARTS", 0);   // >= 2: that many partitions
    int hp_shift = (int)env("QE_HP_SHIFT", 0);   // >= 6: 2^shift buckets per partition
    // buckets per key seen: a wave leaves the probe loop after its LONGEST probe sequence, so the tables are as sparse as the
    // LDS allows (100 000 keys, 256 partitions x 1024 / 2048 / 4096 buckets: 23.4 / 17 / 15.5 ms)
    int hp_fill = (int)env("QE_HP_FILL", 16);
    bool debug_times = std::getenv("QE_DEBUG_TIMES") != nullptr;   // hash-partitioned form: the record array's allocation time to stderr

    static int64_t env(const char *name, int64_t dflt) { const char *v = std::getenv(name); return v ? std::atoll(v) : dflt; }
};
const Knobs &knobs() { static const Knobs k; return k; }

// The profile bracket (ev0 .. ev1, read by collect_time) around a sequence of launches: what launch_fused records around one.
void bracket_open(qe_ctx *ctx) { if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev0, ctx->stream)); }
void bracket_close(qe_ctx *ctx) { if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev1, ctx->stream)); }
float bracket_ms(qe_ctx *ctx) { float ms = 0.f; if (ctx->opts.profile) QE_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1)); return ms; }

// Grid of a kernel that streams the batch's n rows tile by tile, one sub-tile per wave: as many workgroups as there are
// tiles for, at most wgs_per_cu per CU.  `ntiles` (optional): the sub-tiles.
int stream_grid(qe_ctx *ctx, const Plan &plan, int64_t n, int wgs_per_cu, int64_t *ntiles_out = nullptr) {
    const int64_t sub_rows = plan.geo.sub_rows();
    const int64_t ntiles = (n + sub_rows - 1) / sub_rows;
    const int waves = plan.geo.threads / 64;
    if (ntiles_out) *ntiles_out = ntiles;
    return (int)std::max<int64_t>(1, std::min<int64_t>((ntiles + waves - 1) / waves, (int64_t)device_cus(ctx->device) * wgs_per_cu));
}

// qe_ctx_last_groupby_stats (qe_hip.h): run_groupby zeroes the words, a launch that is given up counts itself, and the executor
// that produces the result names its route, the capacity that sufficed and its partitions.
void stats_abandoned(qe_ctx *ctx) { ctx->groupby_stats.w[1]++; }
void stats_route(qe_ctx *ctx, int route, int64_t capacity, int64_t partitions) {
    ctx->groupby_stats.w[0] = route;
    ctx->groupby_stats.w[2] = capacity;
    ctx->groupby_stats.w[3] = partitions;
}

// ---- results built on the host ----------------------------------------------------------------------------------------------
// Column images that asynchronous uploads read: alive until the caller has synchronised the stream.
using HostStaging = std::vector<ColumnImage>;

// One more column of `res`, uploaded from the image of its m rows; a column without a NULL carries no bitmap.
void upload_column(qe_ctx *ctx, qe_result *res, const OutSpec &spec, int64_t m, ColumnImage &&image, HostStaging &keep) {
    keep.push_back(std::move(image));
    const ColumnImage &c = keep.back();
    OutColumn &oc = add_column(ctx, res, spec.type, c.any_null, spec.dict, m);
    if (m == 0) return;
    QE_HIP(hipMemcpyAsync(oc.data, c.values(), column_bytes(spec.type, m), hipMemcpyHostToDevice, ctx->stream));
    if (c.any_null) QE_HIP(hipMemcpyAsync(oc.validity, c.validity(), bitmap_bytes(m), hipMemcpyHostToDevice, ctx->stream));
}

// Key columns of a group-by result: key_of(j, k, word) as key_column_image takes it, for key k of result row j.
template <typename KeyOf>
void append_key_columns(qe_ctx *ctx, const CodegenOutput &cg, qe_result *res, int64_t m, KeyOf key_of, HostStaging &keep) {
    for (int k = 0; k < (int)cg.keys.size(); k++)
        upload_column(ctx, res, cg.keys[k], m, key_column_image(cg.keys[k].type, m, [&](int64_t j, uint64_t &word) { return key_of(j, k, word); }), keep);
}

// Aggregate columns of a group-by result: row j's {first row, (count, acc) per aggregate} words come from `entry_of(j)`.
template <typename EntryOf>
void append_aggregate_columns(qe_ctx *ctx, const CodegenOutput &cg, qe_result *res, int64_t m, EntryOf entry_of, const int32_t *agg_fns, int32_t nagg,
                              HostStaging &keep) {
    for (int i = 0; i < nagg; i++) {
        ColumnImage c = aggregate_column_image(agg_fns[i], i, cg.cnt_src[i], m, entry_of);
        const OutSpec spec{QE_DOUBLE, c.any_null, nullptr};
        upload_column(ctx, res, spec, m, std::move(c), keep);
    }
}

// Key columns of hashed entries: row j's {null bits, key words..} are at `key_words(j)`.
template <typename KeyWords>
void append_hashed_key_columns(qe_ctx *ctx, const CodegenOutput &cg, qe_result *res, int64_t m, KeyWords key_words, HostStaging &keep) {
    append_key_columns(ctx, cg, res, m, [&](int64_t j, int k, uint64_t &word) {
        const uint64_t *e = key_words(j);
        word = e[1 + k];
        return ((e[0] >> k) & 1ull) == 0;
    }, keep);
}

// The groups of a hashed GROUP BY, finished on the host: `dense` holds m entries of cg.hash_words words {state, null bits, key
// words.., first row, (count, acc)..}, listed in insertion order and finished as qe_group_finish.h says.
qe_result *finish_hashed_groups(qe_ctx *ctx, const CodegenOutput &cg, const uint64_t *dense, int64_t m,
                                const int32_t *agg_fns, int32_t nagg) {
    const int W = cg.hash_words, ACC = 2 + (int)cg.keys.size();
    const std::vector<int64_t> order = insertion_order(dense + ACC, (size_t)W, m);
    ResultPtr res = new_result(ctx, m);
    HostStaging keep;
    append_hashed_key_columns(ctx, cg, res.get(), m, [&](int64_t j) { return &dense[(size_t)order[(size_t)j] * W + 1]; }, keep);
    append_aggregate_columns(ctx, cg, res.get(), m, [&](int64_t j) { return &dense[(size_t)order[(size_t)j] * W + ACC]; }, agg_fns, nagg, keep);
    QE_HIP(hipStreamSynchronize(ctx->stream));
    return res.release();
}

// The same on the device, for results of many groups (1 M groups cost the host ~70 ms and crossed the link twice): the entries are
// ordered by first row (their keys = the first rows, a stable LSD radix sort over as many 4-bit digits as the batch's row ids
// have), then one kernel writes every result column -- key values, finished accumulators, validity bitmaps -- in that order.  The
// host only learns which columns hold a NULL anywhere (a column without one carries no bitmap, as the host path decides).
qe_result *finish_hashed_groups_on_device(qe_ctx *ctx, const CodegenOutput &cg, const unsigned long long *d_entries, int64_t m, int64_t nrows,
                                          const int32_t *agg_fns, int32_t nagg) {
    const int W = cg.hash_words, NK = (int)cg.keys.size();
    PoolScratch temps(ctx);
    RadixBuffers rb(temps, m);
    launch_group_sort_keys(ctx->stream, d_entries, W, 2 + NK, m, rb.keys[0], rb.rows[0]);
    int bits = 1;
    while (bits < 62 && (1ll << bits) < nrows) bits++;
    for (int shift = 0; shift < bits; shift += 4) rb.pass(ctx->stream, shift);
    ResultPtr res = new_result(ctx, m);
    GroupFinishArgs a{};
    a.entries = d_entries;
    a.rows = rb.sorted_rows();
    a.m = m;
    a.words = W;
    a.nkeys = NK;
    a.nagg = nagg;
    unsigned int *d_flags = (unsigned int *)temps.alloc(64);
    QE_HIP(hipMemsetAsync(d_flags, 0, 64, ctx->stream));
    a.flags = d_flags;
    // every column gets a bitmap: which of them hold a NULL is known only after the kernel
    for (int k = 0; k < NK; k++) {
        const OutColumn &oc = add_column(ctx, res.get(), cg.keys[k].type, true, cg.keys[k].dict, m);
        a.key_type[k] = oc.type;
        a.key_data[k] = oc.data;
        a.key_valid[k] = (unsigned long long *)oc.validity;
    }
    for (int i = 0; i < nagg; i++) {
        const OutColumn &oc = add_column(ctx, res.get(), QE_DOUBLE, true, nullptr, m);
        a.agg_fn[i] = agg_fns[i];
        a.cnt_src[i] = cg.cnt_src[(size_t)i];
        a.agg_data[i] = (double *)oc.data;
        a.agg_valid[i] = (unsigned long long *)oc.validity;
    }
    launch_group_finish(ctx->stream, a);
    unsigned int flags[16] = {};
    QE_HIP(hipMemcpyAsync(flags, d_flags, 64, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < NK + nagg; c++)   // a column without a NULL carries no bitmap
        if (flags[c < NK ? c : 4 + (c - NK)] == 0) drop_validity(ctx, res->cols[(size_t)c]);
    return res.release();
}

// ---- the partitioned passes ---------------------------------------------------------------------------------------------------
// count -> carry scan -> exclusive prefix on the host -> scatter: the passes that the key-range form (partition = a range of
// dense group ids) and the hash-partitioned form (partition = bits of the key hash) share.  A chunk = subs_per_chunk workgroup
// tiles (one sub-tile per wave each) is the unit both passes hand to a workgroup.  Two steps, because the hash-partitioned form
// decides between them; the caller launches its own aggregate pass over the records and closes the bracket that count() opens.
struct PartitionedPasses {
    qe_ctx *ctx;
    const Plan &plan;
    const int P;                                  // partitions
    PoolScratch temps;                            // counts, starts, the record array -- and what the caller adds
    FusedParams p;
    void *args[1] = {&p};                         // of every launch (points into this object: it is not copied -- temps forbids it)
    hipFunction_t f_scatter = nullptr, f_agg = nullptr;
    int grid = 0;                                 // of the count pass; the scatter pass takes at most as many
    unsigned long long *d_start = nullptr;
    std::vector<unsigned long long> start;        // after count(): start[j] = records before partition j, start[P] = m_records
    unsigned long long m_records = 0;

    PartitionedPasses(qe_ctx *ctx, const Plan &plan) : ctx(ctx), plan(plan), P(plan.cg.nparts), temps(ctx) {}

    void count(const qe_batch *batch) {
        const int64_t chunk_rows = (int64_t)plan.geo.chunk_rows() * (plan.geo.threads / 64);
        const int64_t nchunks = (batch->nrows + chunk_rows - 1) / chunk_rows;
        grid = (int)std::max<int64_t>(1, std::min<int64_t>(nchunks, (int64_t)device_cus(ctx->device) * 8));
        hipFunction_t f_count = nullptr;
        QE_HIP(hipModuleGetFunction(&f_count, plan.kernel.module, "qe_gb_count"));
        QE_HIP(hipModuleGetFunction(&f_scatter, plan.kernel.module, "qe_gb_scatter"));
        QE_HIP(hipModuleGetFunction(&f_agg, plan.kernel.module, "qe_gb_aggregate"));
        uint32_t *d_counts = (uint32_t *)temps.alloc((size_t)nchunks * P * 4);
        d_start = (unsigned long long *)temps.alloc((size_t)(P + 1) * 8);
        fill_inputs(p, batch, plan);
        p.nchunks = nchunks;
        p.blk = (unsigned long long *)d_counts;
        bracket_open(ctx);
        QE_HIP(hipModuleLaunchKernel(f_count, grid, 1, 1, plan.geo.threads, 1, 1, 0, ctx->stream, args, nullptr));
        launch_carry_scan<uint32_t, 256>(ctx->stream, d_counts, nchunks, P, d_start);
        start.assign((size_t)P + 1, 0);
        QE_HIP(hipMemcpyAsync(start.data(), d_start, (size_t)P * 8, hipMemcpyDeviceToHost, ctx->stream));
        QE_HIP(hipStreamSynchronize(ctx->stream));
        for (int j = 0; j < P; j++) {
            const unsigned long long cnt = start[j];
            start[j] = m_records;
            m_records += cnt;
        }
        start[P] = m_records;
    }

    // The records, `record_bytes` for all of them, go to p.desc; nothing is launched when there is no record.  `label` names the
    // form in the diagnostic build's line (debug bit 64: shader clocks per phase, summed over the waves); `times_tag`: the caller wants
    // Knobs::debug_times' line about the record array, under that name.
    void scatter(size_t record_bytes, int wgs_per_cu, const char *label, const char *times_tag = nullptr) {
        QE_HIP(hipMemcpyAsync(d_start, start.data(), (size_t)(P + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (m_records == 0) return;
        p.l1 = d_start;
        const auto t0 = std::chrono::steady_clock::now();
        p.desc = (unsigned long long *)temps.alloc(record_bytes);
        if (times_tag && knobs().debug_times)
            std::fprintf(stderr, "%s: record array of %.2f GB from the pool in %.1f ms\n", times_tag, (double)record_bytes / 1e9,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        const int sgrid = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)device_cus(ctx->device) * (plan.geo.threads >= 512 ? 1 : wgs_per_cu)));
        hipDeviceptr_t dbg = nullptr;
        size_t dbg_bytes = 0;
        if (debug_bit(ctx, kDbgScatterClocks)) {
            QE_HIP(hipModuleGetGlobal(&dbg, &dbg_bytes, plan.kernel.module, "qe_dbg"));
            QE_HIP(hipMemsetAsync(dbg, 0, dbg_bytes, ctx->stream));
        }
        QE_HIP(hipModuleLaunchKernel(f_scatter, sgrid, 1, 1, plan.geo.threads, 1, 1, 0, ctx->stream, args, nullptr));
        if (dbg) {
            unsigned long long h[8] = {};
            QE_HIP(hipMemcpyAsync(h, dbg, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
            QE_HIP(hipStreamSynchronize(ctx->stream));
            const int waves = plan.geo.threads / 64;
            const double waves_total = (double)sgrid * waves;
            std::fprintf(stderr, "qe_gb_scatter%s phases, clocks per wave (grid %d x %d waves): issue loads %.0f | flush (stores) %.0f | "
                         "LDS sort %.0f | wait loads + evaluate %.0f | chunk drain %.0f\n", label, sgrid, waves, h[0] / waves_total,
                         h[1] / waves_total, h[2] / waves_total, h[3] / waves_total, h[4] / waves_total);
        }
    }
};

// GroupByAggregation over a dense group id (dictionary / boolean keys): LDS-privatised table, the partitioned passes by key
// range or global atomics, the groups finished on the host in insertion order.
qe_result *run_groupby_dense(qe_ctx *ctx, const qe_batch *batch, const std::shared_ptr<Plan> &plan, const int32_t *agg_fns, int32_t nagg) {
    const CodegenOutput &cg = plan->cg;
    const int64_t G = cg.ngroups;
    const int W = cg.table_words;
    if (cg.table_copies != 1) fail(QE_ERR_INTERNAL, "dense GROUP BY: a plan with more than one table copy");
    // global accumulator table, initialised from the host (smallest row = ~0, no value seen, accumulators at their identity)
    std::vector<uint64_t> tab((size_t)G * W);
    for (int64_t g = 0; g < G; g++) {
        uint64_t *e = &tab[(size_t)g * W];
        e[0] = ~0ull;
        for (int i = 0; i < nagg; i++) {
            e[1 + 2 * i] = 0;
            e[2 + 2 * i] = agg_identity(agg_fns[i]);
        }
    }
    PoolScratch tab_scratch(ctx);
    unsigned long long *d_tab = (unsigned long long *)tab_scratch.alloc(tab.size() * 8);
    QE_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    const int64_t n = batch->nrows;
    const bool no_partition = debug_bit(ctx, kDbgGroupByGlobalAtomics);   // keep the global-atomic path (A/B measurements, tests)
    if (n > 0 && n < (1ll << 32) && cg.partitioned && !no_partition) {   // record positions are 32-bit in the scatter pass
        // Domain too large for an LDS table: count -> scan -> scatter -> per-partition LDS aggregation
        // (two streaming passes over the input and one over the records instead of one global atomic per value).
        PartitionedPasses pp(ctx, *plan);
        pp.count(batch);
        if (pp.m_records >= (1ull << 32)) fail(QE_ERR_UNSUPPORTED, "partitioned GROUP BY: more than 2^32 records");
        pp.scatter((size_t)(pp.m_records + 16) * 8 * (1 + cg.nvals),   // + the spare line the scatter's idle threads write
                   std::max(1, knobs().scatter_wgs_per_cu), "");
        if (pp.m_records > 0) {
            // pass 3 (generated per plan): slices x P workgroups, one LDS table each, merged into the global table
            const int slices = std::max(1, std::min(64, knobs().agg_wgs / pp.P));
            const int threads = (size_t)cg.part_groups * W * 8 > 48 * 1024 ? 1024 : 256;   // a table that leaves room for one workgroup per CU: make it a big one
            pp.p.agg_partial = (double *)d_tab;
            QE_HIP(hipModuleLaunchKernel(pp.f_agg, slices, pp.P, 1, threads, 1, 1, 0, ctx->stream, pp.args, nullptr));
        }
        bracket_close(ctx);
        QE_HIP(hipStreamSynchronize(ctx->stream));   // the temporaries go back to the pool when this scope ends
        stats_route(ctx, QE_GROUPBY_ROUTE_DENSE_KEY_RANGE, cg.part_groups, pp.P);
    } else if (n > 0) {
        FusedParams p;
        fill_inputs(p, batch, *plan);
        p.agg_partial = (double *)d_tab;
        launch_fused(ctx, *plan, p, stream_grid(ctx, *plan, n, plan->geo.threads >= 1024 ? 1 : 4));   // a 1024-thread workgroup owns its CU (and merges its table once)
        stats_route(ctx, cg.table_in_lds ? QE_GROUPBY_ROUTE_DENSE_LDS : QE_GROUPBY_ROUTE_DENSE_GLOBAL, G, 0);
    } else {
        stats_route(ctx, cg.table_in_lds ? QE_GROUPBY_ROUTE_DENSE_LDS : cg.partitioned && !no_partition ? QE_GROUPBY_ROUTE_DENSE_KEY_RANGE : QE_GROUPBY_ROUTE_DENSE_GLOBAL,
                    cg.partitioned && !no_partition ? cg.part_groups : G, 0);   // nothing to launch: the route the plan stands for
    }
    QE_HIP(hipMemcpyAsync(tab.data(), d_tab, tab.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    if (n > 0) collect_time(ctx);
    const std::vector<int64_t> order = insertion_order(tab.data(), (size_t)W, G);
    const int64_t m = (int64_t)order.size();
    ResultPtr res = new_result(ctx, m);
    HostStaging keep;
    std::vector<int64_t> stride(cg.keys.size(), 1);   // of key k in the group id: the product of the domains (+ NULL code) before it
    for (size_t k = 1; k < cg.keys.size(); k++) stride[k] = stride[k - 1] * (cg.key_domain[k - 1] + 1);
    append_key_columns(ctx, cg, res.get(), m, [&](int64_t j, int k, uint64_t &word) {
        return dense_key_code(order[(size_t)j], stride[(size_t)k], cg.key_domain[(size_t)k], word);
    }, keep);
    append_aggregate_columns(ctx, cg, res.get(), m, [&](int64_t j) { return &tab[(size_t)order[(size_t)j] * W]; }, agg_fns, nagg, keep);
    QE_HIP(hipStreamSynchronize(ctx->stream));
    return res.release();
}

// Hashed group-by whose keys do not fit the LDS table: (1) qe_ht_build gives every key a dense id (global open-addressing
// table, a 64 KiB id cache per workgroup; after its first rows a key is only READ) and writes the id of every kept row;
// (2) the dense group-by -- LDS-privatised table or the partitioned passes -- runs on the id column; (3) the ids of the result
// rows are turned back into key values.  nullptr: more keys than a dense table takes (the caller keeps the global-atomic form).
qe_result *run_groupby_ids(qe_ctx *ctx, const qe_batch *batch, const Plan &plan, const qe_expr *filter, const qe_expr *const *exprs,
                           const int32_t *agg_fns, int32_t nagg, bool *many_keys) {
    const CodegenOutput &cg = plan.cg;
    const int NK = (int)cg.keys.size(), BW = NK == 1 ? 2 : 3 + NK;   // single-key plans: 16-byte entries {key, state | null bits | id}
    const int64_t n = batch->nrows;
    PoolScratch temps(ctx);
    uint32_t *d_ids = (uint32_t *)temps.alloc((size_t)n * 4);
    hipFunction_t f_build = nullptr;
    QE_HIP(hipModuleGetFunction(&f_build, plan.kernel.module, "qe_ht_build"));
    int64_t C = plan.id_capacity > 0 ? plan.id_capacity : (1ll << 16);
    int64_t D = 0;
    unsigned long long *d_keys = nullptr;
    double build_ms = 0.0;
    for (;;) {
        unsigned long long *d_tab = (unsigned long long *)temps.alloc((size_t)C * BW * 8);
        d_keys = (unsigned long long *)temps.alloc((size_t)C * (1 + NK) * 8);
        QE_HIP(hipMemsetAsync(d_tab, 0, (size_t)C * BW * 8, ctx->stream));
        QE_HIP(hipMemsetAsync(ctx->d_ctrl, 0, 96, ctx->stream));
        FusedParams p;
        fill_inputs(p, batch, plan);
        p.agg_partial = (double *)d_tab;
        p.capacity = C;
        p.ticket = ctx->d_ctrl;
        p.error = ctx->d_ctrl + 1;
        p.desc = d_keys;
        p.blk = (unsigned long long *)d_ids;
        void *args[] = {&p};
        bracket_open(ctx);
        QE_HIP(hipModuleLaunchKernel(f_build, stream_grid(ctx, plan, n, 4), 1, 1, plan.geo.threads, 1, 1, 0, ctx->stream, args, nullptr));
        bracket_close(ctx);
        QE_HIP(hipMemcpyAsync(ctx->h_ctrl, ctx->d_ctrl, 32, hipMemcpyDeviceToHost, ctx->stream));
        QE_HIP(hipStreamSynchronize(ctx->stream));
        build_ms += bracket_ms(ctx);
        const unsigned int *hc = (const unsigned int *)ctx->h_ctrl;
        if (hc[1] != 0) {   // more than half full: a bigger table, again (the launch stopped at once: an attempt costs little)
            stats_abandoned(ctx);
            if (many_keys && plan.id_capacity <= 0) {   // the first table of a plan that knows nothing yet: the caller takes over
                *many_keys = true;
                return nullptr;
            }
            if (C >= (1ll << 22)) return nullptr;
            C *= 4;
            continue;
        }
        D = hc[0];
        break;
    }
    plan.id_capacity = C;
    if (D > (1ll << 20) - 1) return nullptr;   // a dense table takes 2^20 groups (the id domain + its NULL code)
    // (2) the dense group-by over [the batch's columns.., ids]: the id column is a dictionary-coded key whose dictionary is a
    // placeholder of 2^k entries (only its size matters: the domain of the group id)
    int64_t dom = 2;
    while (dom < D) dom *= 2;
    dom = std::min<int64_t>(dom, (1ll << 20) - 1);
    std::shared_ptr<DictData> &idd = ctx->id_dicts[dom];
    if (!idd) {
        idd = std::make_shared<DictData>();
        idd->entries.resize((size_t)dom);
    }
    qe_batch tmp;
    tmp.nrows = n;
    tmp.cols = batch->cols;
    for (Column &c : tmp.cols) c.owned = false;
    Column idc;
    idc.type = QE_STRING;
    idc.data = d_ids;
    idc.validity = nullptr;
    idc.dict = idd;
    idc.owned = false;
    tmp.cols.push_back(idc);
    qe_expr kx;
    {
        Node nd;
        nd.kind = N_COLUMN;
        nd.type = QE_STRING;
        nd.col = (int)batch->cols.size();
        kx.e.nodes.push_back(nd);
        kx.e.root = 0;
        kx.e.max_stack = 1;
        const char tag[] = "\xEEid-column";
        kx.e.program.assign(tag, tag + sizeof tag - 1);
        kx.e.program.push_back((uint8_t)batch->cols.size());
    }
    const qe_expr *kp[1] = {&kx};
    auto dplan = get_plan(ctx, &tmp, PlanRequest{filter, exprs, nagg, agg_fns, kp, 1});
    if (dplan->cg.hashed) fail(QE_ERR_INTERNAL, "dense-id plan came out hashed");
    const ResultPtr r = own_result(ctx, run_groupby_dense(ctx, &tmp, dplan, agg_fns, nagg));
    stats_route(ctx, QE_GROUPBY_ROUTE_DENSE_IDS, C, ctx->groupby_stats.w[3]);   // (the partitions are the dense pass's)
    ctx->last_ms += build_ms;   // one step = build pass + dense passes (0 unless profiling; no further launch is counted)
    ctx->total_ms += build_ms;
    // (3) ids of the result rows (column 0, in insertion order) -> key values
    const int64_t m = r->count;
    std::vector<int32_t> rid((size_t)std::max<int64_t>(m, 1));
    std::vector<uint64_t> hkeys((size_t)std::max<int64_t>(D, 1) * (1 + NK));
    if (m > 0) QE_HIP(hipMemcpyAsync(rid.data(), r->cols[0].data, (size_t)m * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (D > 0) QE_HIP(hipMemcpyAsync(hkeys.data(), d_keys, (size_t)D * (1 + NK) * 8, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    ResultPtr res = new_result(ctx, m);
    HostStaging keep;
    append_hashed_key_columns(ctx, cg, res.get(), m, [&](int64_t j) { return &hkeys[(size_t)rid[(size_t)j] * (1 + NK)]; }, keep);
    for (size_t c = 1; c < r->cols.size(); c++) {   // the aggregates move over as they are
        res->cols.push_back(r->cols[c]);
        r->cols[c].data = nullptr;
        r->cols[c].validity = nullptr;
    }
    QE_HIP(hipStreamSynchronize(ctx->stream));
    return res.release();
}

// GroupByAggregation over arbitrary key tuples (a DOUBLE / INT64 / INT32 key, or more key combinations than a dense table
// holds): the hashed form.  Global open-addressing table, grown (x8) and the kernel run again when it got more than half
// full; the used entries are collected on the device and finished on the host (finish_hashed_groups).
// `many_keys` (optional): set -- and nullptr returned, nothing decided for the plan -- when the id build's FIRST table fills up
// (more than 32 768 keys): the caller has a better form for that many keys than a grown id table.
qe_result *run_groupby_hashed(qe_ctx *ctx, const qe_batch *batch, const Plan &plan, const qe_expr *filter, const qe_expr *const *exprs,
                              const int32_t *agg_fns, int32_t nagg, bool *many_keys) {
    const CodegenOutput &cg = plan.cg;
    const bool ids_allowed = !debug_bit(ctx, kDbgHashedGlobalAtomics) && batch->nrows < (1ll << 32);
    bool ids_failed = plan.ids_overflow;   // more keys than a dense table takes, found out by an earlier execution: straight to the global-atomic form
    // The dense-id form.  true: `r` is what this call returns (the result, or nullptr with *many_keys set); false: more keys than
    // a dense table takes -- the global-atomic form after all, and remembered, so that later executions do not run the
    // failing id build again
    qe_result *r = nullptr;
    auto try_ids = [&] {
        r = run_groupby_ids(ctx, batch, plan, filter, exprs, agg_fns, nagg, many_keys);
        if (r || (many_keys && *many_keys)) return true;
        plan.ids_overflow = ids_failed = true;
        plan.use_ids = false;
        return false;
    };
    if (plan.use_ids && ids_allowed && !ids_failed && try_ids()) return r;
    const int W = cg.hash_words, ACC = 2 + (int)cg.keys.size();
    if (W > 40) fail(QE_ERR_UNSUPPORTED, "too many GROUP BY keys + aggregates for one hash entry");
    const int64_t n = batch->nrows;
    HtInit init{};
    init.words = W;
    init.word[ACC] = ~0ull;   // smallest row id
    for (int i = 0; i < nagg; i++) init.word[ACC + 2 + 2 * i] = agg_identity(agg_fns[i]);
    std::vector<uint64_t> dense;
    int64_t m = 0;
    if (n > 0) {
        int64_t C = plan.hash_capacity > 0 ? plan.hash_capacity : (1ll << 16);
        for (;;) {
            PoolScratch tab_scratch(ctx);
            unsigned long long *d_tab = (unsigned long long *)tab_scratch.alloc((size_t)C * W * 8);
            launch_ht_init(ctx->stream, d_tab, C, init);
            QE_HIP(hipMemsetAsync(ctx->d_ctrl, 0, 96, ctx->stream));   // [0] entries in use (p.ticket), [1] error (p.error)
            FusedParams p;
            fill_inputs(p, batch, plan);
            p.agg_partial = (double *)d_tab;
            p.capacity = C;
            p.ticket = ctx->d_ctrl;
            p.error = ctx->d_ctrl + 1;
            p.stagger_chunks = ids_allowed && !ids_failed ? 1 : 0;   // a key that finds no room in LDS stops the launch (error 4) instead of going global
            launch_fused(ctx, plan, p, stream_grid(ctx, plan, n, 4));
            QE_HIP(hipMemcpyAsync(ctx->h_ctrl, ctx->d_ctrl, 16, hipMemcpyDeviceToHost, ctx->stream));
            QE_HIP(hipStreamSynchronize(ctx->stream));
            const unsigned int *hc = (const unsigned int *)ctx->h_ctrl;
            if (hc[1] == 4) {   // the keys do not fit the LDS table: dense ids from now on (this execution included)
                stats_abandoned(ctx);
                plan.use_ids = true;
                if (try_ids()) return r;
                continue;
            }
            collect_time(ctx);
            if (hc[1] != 0) {   // more than half full (or a probe sequence ran out): a bigger table, again
                stats_abandoned(ctx);
                if (C >= (1ll << 28)) fail(QE_ERR_UNSUPPORTED, "GROUP BY produced more than 2^27 groups");
                C *= 8;
                continue;
            }
            plan.hash_capacity = C;
            stats_route(ctx, QE_GROUPBY_ROUTE_HASHED, C, 0);
            const int64_t used = hc[0];
            if (used > knobs().ids_from && ids_allowed && !plan.ids_overflow) plan.use_ids = true;   // the next executions of this plan
            PoolScratch dense_scratch(ctx);   // (goes back to the pool before the table)
            unsigned long long *d_dense = (unsigned long long *)dense_scratch.alloc((size_t)std::max<int64_t>(used, 1) * W * 8);
            QE_HIP(hipMemsetAsync(ctx->d_ctrl, 0, 16, ctx->stream));
            launch_ht_collect(ctx->stream, d_tab, C, W, d_dense, ctx->d_ctrl);
            dense.resize((size_t)used * W);
            if (used > 0) QE_HIP(hipMemcpyAsync(dense.data(), d_dense, dense.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
            QE_HIP(hipGetLastError());
            QE_HIP(hipStreamSynchronize(ctx->stream));
            m = used;
            break;
        }
    }
    if (n == 0) stats_route(ctx, QE_GROUPBY_ROUTE_HASHED, 0, 0);
    return finish_hashed_groups(ctx, cg, dense.data(), m, agg_fns, nagg);
}

// HASH-PARTITIONED form of a hashed GROUP BY with many distinct keys (round 3): count -> scan -> scatter of
// {header, aggregate inputs, key words} records by key HASH (the partitioned passes over a pseudo group id) -> ONE
// workgroup per partition aggregates its records in an LDS hash table and appends the used entries to the result.  Every pass
// streams; no gather, no global atomic per row.  nullptr: a partition held more distinct keys than its table has buckets (the
// caller takes another path and remembers).
// `skewed` (optional) is set, and nullptr returned before the scatter pass, when one partition holds several times its share of
// the records (a key that owns a large part of the rows): ONE workgroup aggregates a partition, so that workgroup would run
// alone for most of the pass -- the dense-id path slices its partitions and does not mind.
qe_result *run_groupby_hp(qe_ctx *ctx, const qe_batch *batch, const std::shared_ptr<Plan> &plan, const int32_t *agg_fns, int32_t nagg,
                          bool *skewed = nullptr) {
    const CodegenOutput &cg = plan->cg;
    const int P = cg.nparts, HW = cg.hash_words;
    PartitionedPasses pp(ctx, *plan);
    pp.count(batch);
    const unsigned long long m_records = pp.m_records;
    if (m_records >= (1ull << 32)) return nullptr;   // record positions are 32-bit in the scatter pass
    if (skewed) {
        unsigned long long largest = 0;
        for (int j = 0; j < P; j++) largest = std::max(largest, pp.start[j + 1] - pp.start[j]);
        if (m_records > (1ull << 22) && largest > 3 * (m_records / (unsigned long long)P) + 65536) {
            *skewed = true;
            stats_abandoned(ctx);
            bracket_close(ctx);   // (the bracket the caller reads must be closed)
            if (ctx->opts.profile) QE_HIP(hipStreamSynchronize(ctx->stream));
            collect_time(ctx);
            return nullptr;
        }
    }
    // whole lines + the spare line, or records + the spare line
    const size_t record_bytes = cg.hp_line_recs ? (size_t)(m_records / cg.hp_line_recs + 2) * 128 : (size_t)(m_records + 16) * 8 * (1 + cg.nvals);
    pp.scatter(record_bytes, kScatterWgsPerCu, " (hash-partitioned)", "run_groupby_hp");
    // the groups' entries come back through pinned staging (64 MB for 1 M groups: 1.5 ms instead of ~15 ms into pageable memory)
    uint64_t *dense = nullptr;
    struct PG { qe_ctx *c; uint64_t **p; ~PG() { if (*p) c->pinned.release(*p); } } pg{ctx, &dense};
    int64_t m = 0;
    if (m_records > 0) {
        const int64_t cap = (int64_t)P * cg.part_groups;   // every bucket of every partition: cannot be exceeded
        unsigned long long *d_out = (unsigned long long *)pp.temps.alloc((size_t)cap * HW * 8);
        pp.p.agg_partial = (double *)d_out;
        pp.p.capacity = cap;
        pp.p.ticket = ctx->d_ctrl;
        pp.p.error = ctx->d_ctrl + 1;
        QE_HIP(hipMemsetAsync(ctx->d_ctrl, 0, 96, ctx->stream));
        QE_HIP(hipModuleLaunchKernel(pp.f_agg, P, 1, 1, 1024, 1, 1, 0, ctx->stream, pp.args, nullptr));
        bracket_close(ctx);
        QE_HIP(hipMemcpyAsync(ctx->h_ctrl, ctx->d_ctrl, 16, hipMemcpyDeviceToHost, ctx->stream));
        QE_HIP(hipStreamSynchronize(ctx->stream));
        collect_time(ctx);
        const unsigned int *hc = (const unsigned int *)ctx->h_ctrl;
        if (hc[1] != 0) {   // 6: some partition's table filled up
            stats_abandoned(ctx);
            return nullptr;
        }
        m = hc[0];
        if (m >= (debug_bit(ctx, kDbgGroupsOnDevice) ? 1 : knobs().groups_on_device_from) && (int)cg.keys.size() <= 4 && nagg <= 8) {
            stats_route(ctx, QE_GROUPBY_ROUTE_HASH_PARTITIONED_DEVICE, cg.part_groups, P);
            return finish_hashed_groups_on_device(ctx, cg, d_out, m, batch->nrows, agg_fns, nagg);
        }
        if (m > 0) {
            dense = (uint64_t *)ctx->pinned.alloc((size_t)m * HW * 8);
            QE_HIP(hipMemcpyAsync(dense, d_out, (size_t)m * HW * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        QE_HIP(hipStreamSynchronize(ctx->stream));
    } else {
        bracket_close(ctx);
        QE_HIP(hipStreamSynchronize(ctx->stream));
        collect_time(ctx);
    }
    stats_route(ctx, QE_GROUPBY_ROUTE_HASH_PARTITIONED_HOST, cg.part_groups, P);
    return finish_hashed_groups(ctx, cg, dense, m, agg_fns, nagg);
}

// ---- hashed GROUP BY: the choice of the route -----------------------------------------------------------------

// the widest table a partition of the hash-partitioned form may have, as log2 of its buckets: entry = {first row, key words..,
// the counters and accumulators the plan needs}: {first row, key, MIN, MAX} and {first row, key, count, SUM} are 32 bytes:
// 4096 buckets in 128 KiB
int hp_max_shift(const AggregateCall &q, const CodegenOutput &cg) {
    int max_shift = 12;
    bool keys_nullable = false;
    std::vector<char> agg_nullable;
    for (int i = 0; i < q.nagg; i++) agg_nullable.push_back(cg.outs[(size_t)i].nullable ? 1 : 0);
    for (const OutSpec &ks : cg.keys) keys_nullable = keys_nullable || ks.nullable;
    const int64_t entry_bytes = 8 * (1 + q.nkeys + (keys_nullable ? 1 : 0) + hp_entry_layout(agg_nullable, q.agg_fns, q.nagg).words);
    while (max_shift > 8 && (entry_bytes << max_shift) > 144 * 1024) max_shift--;
    return max_shift;
}

// one attempt at the hash-partitioned form with P partitions of 2^shift buckets: the result, or nullptr when some partition's
// table filled up (or the form is not to be had: plan->hp_failed)
qe_result *try_hp(const AggregateCall &q, const std::shared_ptr<Plan> &plan, int P, int shift) {
    std::shared_ptr<Plan> hplan;
    try {
        PlanRequest rq = q.request();
        rq.hp_parts = P;
        rq.hp_shift = shift;
        hplan = get_plan(q.ctx, q.batch, rq);
    } catch (const Error &) {   // e.g. an entry too wide for the LDS table: the other forms stay
        plan->hp_failed = true;
        return nullptr;
    }
    if (!hplan || !hplan->cg.hp) return nullptr;
    qe_result *r = nullptr;
    bool skewed = false;
    try {
        r = run_groupby_hp(q.ctx, q.batch, hplan, q.agg_fns, q.nagg, &skewed);
    } catch (const Error &e) {
        // its record array (21 - 64 bytes per kept row) did not fit beside the batch: the dense-id path needs 4 + 16
        // bytes per row -- this plan stays with that one (run_groupby_hp releases what it had allocated)
        if (e.code != QE_ERR_OOM) throw;
        plan->hp_failed = true;
    }
    if (skewed) plan->hp_failed = true;   // a property of the data: this plan stays with the forms that slice their work
    if (r) {
        plan->known_keys = r->count;
        q.ctx->last_form = QE_FORM_GROUPBY_HASH_PARTITIONED;
    }
    return r;
}

qe_result *run_groupby_hashed_route(const AggregateCall &q, const std::shared_ptr<Plan> &plan) {
    qe_ctx *ctx = q.ctx;
    const qe_batch *batch = q.batch;
    // many distinct keys (known from an earlier execution of this plan, Knobs::hp_from): the hash-partitioned form -- every pass
    // streams -- instead of the id build + dense passes (100 000 DOUBLE keys, 1 B rows: 24 ms that way)
    const Knobs &kn = knobs();
    const bool hp_forced = debug_bit(ctx, kDbgForceHashPartitioned), hp_never = debug_bit(ctx, kDbgNeverHashPartitioned);
    const int64_t n = batch->nrows;
    const bool hp_possible = !hp_never && !plan->hp_failed && n > 0 && n < (1ll << 32) && q.nkeys <= 4 && q.nagg <= 8;
    const int max_shift = hp_max_shift(q, plan->cg);
    // ONE workgroup aggregates a partition (128 partitions left half the chip idle: 21.8 ms for the aggregation of 1 B
    // records).  Fewer partitions make longer runs per scatter tile -- less padding to whole lines --, more partitions keep
    // the tables sparse.  Buckets for ~16x the keys seen (Knobs::hp_fill), 256 .. 4096 per partition.
    // few partitions = long runs per scatter tile = little padding, and the probe loop tolerates full tables better than the
    // scatter tolerates short runs (1 M keys, 1 B rows: 512 partitions half full 24.6 ms, 1024 partitions a quarter full
    // 37.1 ms; 500 000 keys: 256 partitions half full 22.6 ms, 512 a quarter full 18.3 ms): 256 partitions up to 30 %, 512
    // up to 50 %, 1024 beyond
    struct HpSize { int P, shift; };
    auto size_for = [&](int64_t known_keys) {
        const int64_t keys_seen = std::max<int64_t>(known_keys, 1);
        HpSize z{keys_seen * 10 <= ((int64_t)256 << max_shift) * 3 ? 256 : keys_seen * 2 <= ((int64_t)512 << max_shift) ? 512 : 1024, 8};
        if (hp_forced && known_keys <= 0) z.P = 64;
        if (kn.hp_parts >= 2) z.P = kn.hp_parts;
        while (z.shift < max_shift && ((int64_t)z.P << z.shift) < keys_seen * kn.hp_fill) z.shift++;
        if (kn.hp_shift >= 6) z.shift = kn.hp_shift;
        return z;
    };
    HpSize overflowed{0, 0};   // partitions that were sized from a key count and overflowed in this execution
    if (hp_possible && (hp_forced || (plan->known_keys >= kn.hp_from && n >= (4ll << 20)))) {
        const HpSize z = size_for(plan->known_keys);
        if (qe_result *r = try_hp(q, plan, z.P, z.shift)) return r;
        // some partition's table filled up: with 1024 partitions there is nothing larger to try; otherwise the run below
        // reports how many keys there are and the next execution sizes its partitions from that
        if (z.P >= 1024) plan->hp_failed = true;
        else if (plan->known_keys > 0 && kn.hp_parts < 2 && kn.hp_shift < 6) overflowed = z;
    }
    // The FIRST execution of a plan does not know its keys.  The LDS tables and the id build find out cheaply that there are
    // many (their launches stop at once when a table fills up: more than 32 768 keys fill the id build's first table); from
    // there the hash-partitioned form takes over with the widest tables -- 256, then 512, then 1024 partitions when a table
    // overflows -- instead of growing the id table (100 000 keys, 1 B rows: a first execution of 48 ms that way).
    bool many_keys = false;
    const bool first_hp = hp_possible && !hp_forced && plan->known_keys < 0 && plan->id_capacity <= 0 && n >= (4ll << 20);
    qe_result *out = run_groupby_hashed(ctx, batch, *plan, q.filter, q.exprs, q.agg_fns, q.nagg, first_hp ? &many_keys : nullptr);
    if (!out && many_keys) {
        for (int P = 256; P <= 1024 && !out && !plan->hp_failed; P *= 2) out = try_hp(q, plan, P, max_shift);
        if (out) return out;
        out = run_groupby_hashed(ctx, batch, *plan, q.filter, q.exprs, q.agg_fns, q.nagg, nullptr);   // more keys than 1024 tables hold
    }
    if (out) plan->known_keys = out->count;
    // .. unless that count sizes the very partitions that have just overflowed (the count was exact already: these keys crowd
    // into one partition whatever its table): every later execution would repeat count pass, scatter pass and the abandoned
    // aggregation before it falls back -- the plan gives the form up
    if (out && overflowed.P > 0) {
        const HpSize again = size_for(plan->known_keys);
        if (again.P == overflowed.P && again.shift == overflowed.shift) plan->hp_failed = true;
    }
    ctx->last_form = QE_FORM_GROUPBY_HASHED;
    return out;
}

}  // namespace

namespace qe {

qe_result *run_groupby(const AggregateCall &q) {
    q.ctx->groupby_stats.store(0, 0, 0, 0);
    auto plan = get_plan(q.ctx, q.batch, q.request());
    if (plan->cg.hashed) return run_groupby_hashed_route(q, plan);
    qe_result *out = run_groupby_dense(q.ctx, q.batch, plan, q.agg_fns, q.nagg);
    q.ctx->last_form = QE_FORM_GROUPBY_DENSE;
    return out;
}

// The global aggregate: every workgroup leaves {(acc, count) per aggregate, selected rows}, folded on the host.
void run_global_aggregate(const AggregateCall &q, double *out_values, uint8_t *out_valid, int64_t *out_selected_rows) {
    qe_ctx *ctx = q.ctx;
    const qe_batch *batch = q.batch;
    auto plan = get_plan(ctx, batch, q.request());
    // fixed grid => fixed reduction tree => bitwise reproducible sums on a given device
    int64_t ntiles = 0;
    const int grid = stream_grid(ctx, *plan, batch->nrows, 8, &ntiles);
    std::vector<double> partial((size_t)grid * (2 * q.nagg + 1), 0.0);
    if (ntiles > 0) {
        FusedParams p;
        fill_inputs(p, batch, *plan);
        PoolScratch scratch(ctx);
        double *d_partial = (double *)scratch.alloc(partial.size() * 8);
        p.agg_partial = d_partial;
        p.nchunks = ntiles;
        launch_fused(ctx, *plan, p, grid);
        QE_HIP(hipMemcpyAsync(partial.data(), d_partial, partial.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        QE_HIP(hipStreamSynchronize(ctx->stream));
        collect_time(ctx);
    }
    const int64_t nsel = fold_global_partials(partial.data(), ntiles > 0 ? grid : 0, q.agg_fns, q.nagg, out_values, out_valid);
    if (out_selected_rows) *out_selected_rows = nsel;
}

}  // namespace qe

extern "C" {

int32_t qe_filter_aggregate_prepare(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                    const qe_expr *const *exprs, const int32_t *agg_fns, int32_t nagg) {
    if (!ctx || !batch || nagg <= 0 || !exprs || !agg_fns) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        if (ctx->device >= 0) need_device(ctx);
        const AggregateCall q{ctx, batch, filter, nullptr, 0, exprs, agg_fns, nagg};
        (void)get_plan(ctx, batch, q.request(ctx->device >= 0));
    });
}

int32_t qe_filter_aggregate(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter, const qe_expr *const *exprs,
                            const int32_t *agg_fns, int32_t nagg, double *out_values, uint8_t *out_valid,
                            int64_t *out_selected_rows) {
    if (!ctx || !batch || nagg <= 0 || !exprs || !agg_fns || !out_values || !out_valid) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        need_device(ctx);
        if (batch->schema_only) fail(QE_ERR_INVALID_ARG, "schema-only batch (qe_batch_describe) cannot be executed");
        run_global_aggregate({ctx, batch, filter, nullptr, 0, exprs, agg_fns, nagg}, out_values, out_valid, out_selected_rows);
    });
}

int32_t qe_filter_groupby_prepare(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter, const qe_expr *const *keys,
                                  int32_t nkeys, const qe_expr *const *exprs, const int32_t *agg_fns, int32_t nagg) {
    if (!ctx || !batch || nkeys <= 0 || !keys || nagg <= 0 || !exprs || !agg_fns) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        if (ctx->device >= 0) need_device(ctx);
        const AggregateCall q{ctx, batch, filter, keys, nkeys, exprs, agg_fns, nagg};
        PlanRequest rq = q.request(ctx->device >= 0);
        auto plan = get_plan(ctx, batch, rq);
        if (plan->cg.hashed && debug_bit(ctx, kDbgForceHashPartitioned) && nkeys <= 4 && nagg <= 8) {   // forced hash-partitioned form: its plan too
            rq.hp_parts = 64;
            rq.hp_shift = 8;
            (void)get_plan(ctx, batch, rq);
        }
    });
}

int32_t qe_filter_groupby(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter, const qe_expr *const *keys, int32_t nkeys,
                          const qe_expr *const *exprs, const int32_t *agg_fns, int32_t nagg, qe_result **out) {
    if (!ctx || !batch || !out || nkeys <= 0 || !keys || nagg <= 0 || !exprs || !agg_fns) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(ctx, [&] {
        need_device(ctx);
        if (batch->schema_only) fail(QE_ERR_INVALID_ARG, "schema-only batch (qe_batch_describe) cannot be executed");
        *out = run_groupby({ctx, batch, filter, keys, nkeys, exprs, agg_fns, nagg});
    });
}

int32_t qe_ctx_last_groupby_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::groupby_stats, out); }

}  // extern "C"
