// qe_api.cpp -- the executor that picks form / order / geometry: the plan cache and the geometry a plan settles on
// (get_plan), the filter+project executor (run_fused: a form choice and one function per form) and its entry points.
// The rest of the C ABI lives in qe_context.cpp, qe_groupby.cpp and qe_result.cpp (map: qe_exec.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <sstream>

#include "qe_exec.h"
#include "qe_kernels.h"
#include "qe_pernode.h"
#include "qe_scan.h"

using namespace qe;

// ---- plans --------------------------------------------------------------------------------------------
namespace {

// a plan that kept at least this share of its rows last time runs the dense single-pass kernel next time (measured
// crossover against the LDS-ring kernel on cfg 2, 1 B rows: 10 % 4.14 vs 4.23 ms, 25 % 5.7 vs 4.5 ms)
constexpr double kDenseFromSelectivity = 0.12;
// a plan that kept at most this share of its rows last time runs the LOCAL form next time: scan without any inter-wave
// dependency into per-chunk slots, then a scan over the counts and one move
constexpr double kLocalUpToSelectivity = 0.03;
constexpr int64_t kSampleFromRows = 8ll << 20;   // batches from here on sample their selectivity before the first execution of a plan

FusedGeometry geometry_of(const qe_ctx *ctx) {
    FusedGeometry g;
    const int t = ctx->opts.tuning[0], u = ctx->opts.tuning[1];
    if (t == 64 || t == 128 || t == 256 || t == 512 || t == 1024) g.threads = t;
    const int mw = ctx->opts.tuning[3] / 100;    // tuning[3] = 100 * min_waves + blocks_per_cu
    if (mw >= 1 && mw <= 8) g.min_waves = mw;
    if (u >= 1 && u <= 16) g.unroll = u;
    const int spc = ctx->opts.tuning[4] % 10000;   // tuning[4] = subs_per_chunk + 10000 * (LDS ring entries / 256)
    if (spc >= 1 && spc <= 4096) g.subs_per_chunk = spc;
    const int ringk = ctx->opts.tuning[4] / 10000;
    if (ringk == 1 || ringk == 2 || ringk == 4) g.ring_entries = 256 * ringk;
    const int lbk = ctx->opts.tuning[6] % 100;   // tuning[6] = lookback_k + 100 * gate_period_log2 + 10000 * gate_width_log2
    if (lbk >= 1 && lbk <= 16) g.lookback_k = lbk;
    const int gp = (ctx->opts.tuning[6] / 100) % 100, gw = ctx->opts.tuning[6] / 10000;
    if (gp >= 8 && gp <= 24 && gw >= 4 && gw < gp) { g.gate_period_log2 = gp; g.gate_width_log2 = gw; }
    const int pm = ctx->opts.tuning[2] / 10;   // tuning[2] = 10 * (prio_mode + 1) + nt ; 0 = default
    if (pm >= 1 && pm <= 4) g.prio_mode = pm - 1;   // 0 none, 1 per sub-tile mod 3, 2 per chunk mod 3, 3 per sub-tile mod 2
    const int nb = ctx->opts.tuning[7] / 100;   // tuning[7] = 100 * nbuf + (stagger / resolve_at code)
    if (nb >= 2 && nb <= 8) g.nbuf = nb;
    const int st7 = ctx->opts.tuning[7] % 100;
    if (st7 == 2) g.stagger = 0;
    if (st7 == 1 && g.subs_per_chunk % 16 == 0) g.stagger = 1;
    if (st7 >= 10) g.resolve_at = st7 - 10;   // 10 + n: resolve n sub-tiles into the next chunk
    return g;
}

// The geometry steps of get_plan, in the order it calls them (later steps read what earlier ones set).  They settle in.geo
// (and in.hp_lines) from plan->cg, which holds the generator's ANALYSIS of `in` here: no text is written before a compile.
struct PlanGeometry {
    qe_ctx *ctx;
    CodegenInput &in;
    Plan *plan;
    const bool wide;
    const int32_t *agg_fns;
    void analyze() { plan->cg = analyze_fused_plan(in); }
    void narrow_plan_wide_candidate();
    void lds_table_1024_threads();
    void hash_partitioned_tile();
    void partitioned_tile_512_threads();
    void hashed_unroll();
    void dense_lds_tile();
    void ring_lds_budget();
    void register_estimate();
    void compile_without_scratch();
};


}  // namespace

namespace qe {

std::shared_ptr<Plan> get_plan(qe_ctx *ctx, const qe_batch *batch, const PlanRequest &rq) {
    if (rq.nproj < 0 || (rq.nproj > 0 && !rq.projs)) fail(QE_ERR_INVALID_ARG, "bad projection list");
    CodegenInput in;
    in.filter = rq.filter ? &rq.filter->e : nullptr;
    for (int32_t i = 0; i < rq.nproj; i++) {
        if (!rq.projs[i]) fail(QE_ERR_INVALID_ARG, "null projection");
        in.projections.push_back(&rq.projs[i]->e);
        if (rq.agg_fns) {
            if (rq.agg_fns[i] < QE_AGG_MIN || rq.agg_fns[i] > QE_AGG_AVG) fail(QE_ERR_UNSUPPORTED, "unsupported aggregation function");
            in.agg_fns.push_back(rq.agg_fns[i]);
        }
    }
    for (int32_t i = 0; i < rq.nkeys; i++) {
        if (!rq.keys || !rq.keys[i]) fail(QE_ERR_INVALID_ARG, "null group key");
        in.group_keys.push_back(&rq.keys[i]->e);
    }
    in.cmp_semantics = ctx->opts.cmp_semantics;
    if (rq.conj_order) in.conj_order = *rq.conj_order;
    in.hp_parts = rq.hp_parts;
    // records in 128-byte lines pad in units of 6 / 4 / 3 / 2 where {header, words} records of 32 bytes pad in units of 4: they win
    // while a scatter tile holds runs of several records per partition (1 B rows, SELECT k, MIN(v), MAX(v), lines / records: 256
    // partitions, 100 000 keys 16.9 / 18.3 ms; 512 partitions, 500 000 keys 18.3 / 20.6, 1 M keys 24.6 / 26.7); with 1024 partitions
    // the stage of a tile's lines no longer fits a 4 Ki-row tile.  kDbgHpRecords: always {header, words} records.
    static const int lines_maxp = std::getenv("QE_HP_LINES_MAXP") ? std::atoi(std::getenv("QE_HP_LINES_MAXP")) : 512;
    in.hp_lines = !debug_bit(ctx, kDbgHpRecords) && rq.hp_parts <= lines_maxp ? 1 : 0;
    in.hp_shift = rq.hp_shift;
    in.geo = geometry_of(ctx);
    const bool wide = rq.geo_cand == 1;
    if (wide) {   // the second candidate of the geometry choice (qe_ctx::geo_choice)
        in.geo.unroll = 16;
        in.geo.subs_per_chunk = 4;
        in.geo.ring_entries = 512;
    } else if (rq.geo_cand == 2) {
        // the third candidate (round 3): the default sub-tile, 8 Ki-row chunks whose kept rows fit 512-entry rings, two waves per
        // workgroup.  cfg 2, 1 B rows, three boxes: default / wide / this = 3.56 / 3.29 / 3.19, 3.47 / 3.47 / 3.19 and
        // (a fast box) 3.35 / 3.13 / 3.20 ms -- which one wins depends on the box, so it is measured like the other two
        in.geo.unroll = 8;
        in.geo.subs_per_chunk = 8;
        in.geo.ring_entries = 512;
        in.geo.threads = 128;
    }
    in.nontemporal = ctx->opts.tuning[2] % 10 == 2 ? 0 : 1;
    in.vec_stores = ctx->opts.tuning[2] % 10 == 5 ? 1 : 0;   // tuning[2] % 10 == 5: 16-byte output stores (measurement)
    in.nt_stores = ctx->opts.tuning[2] % 10 == 3 ? 0 : ctx->opts.tuning[2] % 10 == 4 ? 2 : 1;   // tuning[2] % 10: 2 plain loads, 3 plain output stores, 4 nt spill stores too
    in.debug_mask = ctx->opts.tuning[5] & kDbgAblationMask;   // the other bits are host-side switches, not ablation builds
    in.staged = !debug_bit(ctx, kDbgNoLateMaterialisation);
    in.prefetch = debug_bit(ctx, kDbgNoPrefetch) ? 0 : debug_bit(ctx, kDbgAlwaysPrefetch) ? 2 : 1;   // stage-0 prefetch: never / always
    in.dense = rq.dense && rq.filter != nullptr && !rq.agg_fns;
    if (in.dense) {   // the dense kernel has its own shape: a workgroup per tile of QE_WAVES sub-tiles, one tile parked in LDS
        in.geo.subs_per_chunk = 1;
        in.geo.stagger = 0;
        // measured on cfg 2, 1 B rows (tools/sel_sweep.py): 4 waves x 1024 rows = 4 Ki-row tiles (244 K tickets, 64 KiB of LDS
        // for 16-byte rows, two workgroups per CU) ran 4.0 - 6.4 ms from 1 % to 100 %; 2 Ki-row tiles are bound by the
        // single-address ticket rate (~77 tickets/us: 6.3 ms whatever the selectivity), 8 / 16 Ki-row tiles leave one
        // workgroup per CU (5 - 15 % slower)
        if (ctx->opts.tuning[0] == 0) in.geo.threads = 256;
        if (ctx->opts.tuning[1] == 0) in.geo.unroll = 8;
    }
    in.filter_load_stages = debug_bit(ctx, kDbgOneFilterLoadStage) ? 1 : 0;
    std::ostringstream key;
    key << "m" << (rq.agg_fns ? 1 : 0) << (in.dense ? "D" : "") << "c" << in.cmp_semantics << "t" << in.geo.threads << "u" << in.geo.unroll << "s"
        << in.geo.subs_per_chunk << "n" << in.nontemporal << in.nt_stores << in.vec_stores << "L" << (in.staged ? 1 : 0) << "P" << in.prefetch << "." << in.filter_load_stages << "k" << in.geo.lookback_k << "G" << in.geo.gate_period_log2 << "." << in.geo.gate_width_log2 << "d" << in.debug_mask << "r" << in.geo.resolve_at << "g" << in.geo.stagger << "w" << in.geo.min_waves << "p" << in.geo.prio_mode << "b" << in.geo.nbuf << "R" << in.geo.ring_entries << "|";
    for (const Column &c : batch->cols) {
        in.schema.push_back(BoundColumn{c.type, c.validity != nullptr, c.dict});
        key << c.type << (c.validity ? 'n' : 'v') << (c.dict ? c.dict->id : 0) << ",";   // the dictionary's serial number, not its address
    }
    auto add_prog = [&](const Expr *e) {
        key << "|";
        if (e) key.write((const char *)e->program.data(), (std::streamsize)e->program.size());
    };
    add_prog(in.filter);
    for (const Expr *e : in.projections) add_prog(e);
    for (const Expr *e : in.group_keys) {
        key << "|k";
        add_prog(e);
    }
    if (rq.agg_fns)
        for (int a : in.agg_fns) key << "|a" << a;
    if (in.hp_parts) key << "|H" << in.hp_parts << "." << in.hp_shift << "." << in.hp_lines;
    if (!in.conj_order.empty()) {
        key << "|O";
        for (int o : in.conj_order) key << o << ".";
    }
    const std::string k = key.str();
    auto it = ctx->plans.find(k);
    if (it != ctx->plans.end() && (it->second->kernel.fn || !rq.load)) return it->second;
    auto plan = std::make_shared<Plan>();
    PlanGeometry pg{ctx, in, plan.get(), wide, rq.agg_fns};
    pg.analyze();
    pg.narrow_plan_wide_candidate();
    pg.lds_table_1024_threads();
    pg.hash_partitioned_tile();
    pg.partitioned_tile_512_threads();
    pg.hashed_unroll();
    pg.dense_lds_tile();
    pg.ring_lds_budget();
    if (ctx->opts.tuning[3] / 100 == 0) {
        pg.register_estimate();
        pg.compile_without_scratch();
    } else {
        plan->cg = generate_fused_source(in);
    }
    plan->geo = in.geo;
    plan->explicit_geometry = ctx->opts.tuning[0] != 0 || ctx->opts.tuning[1] != 0 || ctx->opts.tuning[3] != 0 || ctx->opts.tuning[4] != 0 ||
                              ctx->opts.tuning[7] != 0;
    plan->aggregate = rq.agg_fns != nullptr;
    plan->kernel = ctx->jit->get(plan->cg.source, "qe_fused", rq.load);
    ctx->plans[k] = plan;
    return plan;
}

}  // namespace qe

namespace {

void PlanGeometry::narrow_plan_wide_candidate() {
    if (wide && !in.dense && !agg_fns && in.group_keys.empty()) {
        // A plan that reads few bytes per row (cfg 4: a 4-byte code and an 8-byte value) pays the per-chunk work -- ticket,
        // descriptors, look-back -- on few bytes: its second candidate keeps the 16 load groups but hands out 32 Ki-row chunks
        // (16 sub-tiles) with the default rings instead of 8 Ki-row chunks.  Measured on cfg 4, 1 B rows: default 1.02 ms,
        // 16 groups x 4 sub-tiles 0.97 ms, 16 groups x 16 sub-tiles 0.80 ms.  The choice itself stays measured (best of 3).
        size_t inbytes = 0;
        for (int c : plan->cg.used_cols) inbytes += (size_t)value_bytes(in.schema[(size_t)c].type);
        if (inbytes <= 16) {
            const FusedGeometry dflt = geometry_of(ctx);
            in.geo.subs_per_chunk = dflt.subs_per_chunk;
            in.geo.ring_entries = dflt.ring_entries;
        }
    }
}

void PlanGeometry::lds_table_1024_threads() {
    if (!in.group_keys.empty() && !plan->cg.hashed && !plan->cg.table_in_lds && ctx->opts.tuning[0] == 0 &&
        (size_t)plan->cg.ngroups * plan->cg.table_words * 8 <= 144 * 1024) {
        in.geo.threads = 1024;   // the table fits ONE workgroup's LDS: 16 waves per CU share it (see table_in_lds)
        analyze();
    }
}

void PlanGeometry::hash_partitioned_tile() {
    if (plan->cg.hp && ctx->opts.tuning[1] == 0 && ctx->opts.tuning[0] == 0) {
        // the scatter pass sorts a workgroup tile's records in ONE LDS stage: 8 waves x 512 rows x 32-byte records = 128 KiB (one
        // workgroup per CU) was the fastest of the shapes measured on 100 000 DOUBLE keys, 512 partitions: 4 waves x 1024 rows
        // 31.4 ms, 4 x 512 29.0, 8 x 512 25.6, 8 x 256 29.3; wider records take fewer rows per wave
        in.geo.threads = 512;
        int u = 4;
        auto lines_lds = [&](int uu) {   // the stage holds the tile's LINES: every partition's run padded to whole lines, in the worst case
            const size_t R = (size_t)std::max(1, plan->cg.hp_line_recs), P = (size_t)plan->cg.nparts;
            const size_t tile = (size_t)(in.geo.threads / 64) * 128 * uu, lines = (tile + (P <= 256 ? 2 : 1) * (R - 1) * P + R - 1) / R;
            return lines * 132 + ((P + 3) & ~(size_t)3) * (P <= 256 ? 24 : 16) + 64;   // (<= 256 partitions: the carry -- every run may also START with waiting records)
        };
        if (plan->cg.hp_line_recs && lines_lds(4) > 156 * 1024) {
            // wide records (two or three per line) in many partitions: the lines' stage would force a smaller tile, i.e. shorter runs and
            // more padding than the {header, words} records have
            in.hp_lines = 0;
            analyze();
        }
        if (plan->cg.hp_line_recs) {
            while (u > 1 && lines_lds(u) > 156 * 1024) u /= 2;
        } else {
            const size_t rec = (size_t)(1 + plan->cg.nvals) * 8;
            while (u > 1 && (size_t)(in.geo.threads / 64) * 128 * u * rec > 128 * 1024) u /= 2;
        }
        in.geo.unroll = u;
    }
}

void PlanGeometry::partitioned_tile_512_threads() {
    if (plan->cg.partitioned && !plan->cg.hp && plan->cg.nparts > 128 && ctx->opts.tuning[0] == 0 && in.geo.threads == 256 &&
        8 + plan->cg.part_shift + 13 <= 32 && (size_t)8 * in.geo.sub_rows() * (1 + plan->cg.nvals) * 8 <= 128 * 1024) {
        // many partitions: a tile of 8 waves (8 Ki rows, one workgroup per CU) holds twice the records per partition, so the
        // whole-line padding of the scatter pass costs half as much (1 M keys: 45 % -> 22 % more records)
        in.geo.threads = 512;
    }
}

void PlanGeometry::hashed_unroll() {
    if (plan->cg.hashed && ctx->opts.tuning[1] == 0 && in.geo.unroll > 4) {
        in.geo.unroll = 4;   // hashed group-by: the key words of 2 * U rows live in registers next to the inputs; it is bound by atomics, not by loads in flight
    }
}

void PlanGeometry::dense_lds_tile() {
    if (in.dense) {
        // LDS budget of the parked tile: (waves * 128 * U) rows of every output column.  64 KiB lets two workgroups share a
        // CU (the second one streams while the first waits at its barriers); shrink the sub-tile, then the workgroup.
        const size_t rowbytes = std::max<size_t>(output_row_bytes(plan->cg.outs), 1);
        auto tile_bytes = [&]() { return (size_t)(in.geo.threads / 64) * 128 * in.geo.unroll * rowbytes; };
        const size_t limit = 64 * 1024;
        while (tile_bytes() > limit && in.geo.unroll > 1 && ctx->opts.tuning[1] == 0) in.geo.unroll /= 2;
        while (tile_bytes() > limit && in.geo.threads > 128 && ctx->opts.tuning[0] == 0) in.geo.threads /= 2;
        if (tile_bytes() > 150 * 1024)
            fail(QE_ERR_UNSUPPORTED, "projection list too wide for the dense kernel's LDS tile (" + std::to_string(rowbytes) + " bytes per output row)");
    }
}

void PlanGeometry::ring_lds_budget() {
    if (!agg_fns && in.filter && !in.dense) {
        // LDS budget of the per-wave FIFO of chunk buffers: waves * nbuf * ring * (bytes per output row).
        // Narrow rows get 3 buffers; wide rows 2 buffers and, if need be, fewer waves per workgroup so that a
        // workgroup stays within the 160 KiB of a CU (and several workgroups still fit).
        const size_t rowbytes = std::max<size_t>(output_row_bytes(plan->cg.outs), 1);
        if (ctx->opts.tuning[7] / 100 == 0) in.geo.nbuf = 2;
        if (ctx->opts.tuning[0] == 0) {
            const size_t limit = 96 * 1024;
            while (in.geo.threads > 64 && (size_t)(in.geo.threads / 64) * in.geo.nbuf * in.geo.ring_entries * rowbytes > limit)
                in.geo.threads /= 2;
        }
        if ((size_t)(in.geo.threads / 64) * in.geo.nbuf * in.geo.ring_entries * rowbytes > 156 * 1024)
            fail(QE_ERR_UNSUPPORTED, "projection list too wide for the fused kernel's LDS buffers (" + std::to_string(rowbytes) +
                                         " bytes per output row); use QE_EXEC_PER_NODE");
    }
}

void PlanGeometry::register_estimate() {
    // Register budget.  Per lane a sub-tile holds 2*U rows of every input column, later of every output
    // column, plus one VGPR per boolean per row: shrink the sub-tile of very wide plans first.  Then ask
    // for the highest occupancy (__launch_bounds__ waves per SIMD) that compiles WITHOUT SCRATCH: a spill
    // turns into HBM traffic (84 B/lane of scratch cost 2.7 GB of extra writes per 1 B rows when measured).
    auto dwords = [](int t) { return (t == QE_DOUBLE || t == QE_INT64) ? 2 : 1; };
    for (;;) {
        int in_dw = 0, out_dw = 0, nbool = 1, in_nulls = 0;
        for (int c : plan->cg.used_cols) {
            in_dw += dwords(in.schema[c].type);
            in_nulls += in.schema[c].nullable ? 1 : 0;
        }
        for (const OutSpec &o : plan->cg.outs) {
            out_dw += dwords(o.type);
            nbool += o.nullable ? 1 : 0;
        }
        // the validity bits of ALL nullable inputs share one register per load group (qe_vb)
        const int est = 2 * in.geo.unroll * (std::max(in_dw, out_dw) + nbool - 1) + (in_nulls ? in.geo.unroll : 0) + 54;
        // three waves per SIMD need <= 168 VGPRs: a half-size sub-tile at 3 waves beat the full one at 2 waves
        // (cfg 2 with nullable inputs: 4.47 vs 6.16 ms per 1 B rows)
        plan->est_regs = est;
        if (((est > 168 && in.geo.unroll > 4) || (est > 300 && in.geo.unroll > 2)) && ctx->opts.tuning[1] == 0 && !wide) {
            in.geo.unroll /= 2;
            if (!in.dense) in.geo.subs_per_chunk *= 2;   // keep the chunk size (the dense kernel's chunk IS the sub-tile)
            continue;
        }
        // (nullable cfg 2, est 122: 3 waves per SIMD 3.54 ms, 4 waves 3.69 ms -- the request also shapes the register allocation)
        in.geo.min_waves = est <= 120 ? 4 : est <= 168 ? 3 : est <= 256 ? 2 : 1;
        break;
    }
}

// compile (or hit the cache) at the estimated geometry; while the code object spills, ask for less and generate again
void PlanGeometry::compile_without_scratch() {
    for (;;) {
        plan->cg = generate_fused_source(in);
        plan->kernel = ctx->jit->get(plan->cg.source, "qe_fused", false);   // compile (or cache hit) only
        if (ctx->jit->last_scratch <= 0) break;
        const bool can_retry = in.geo.min_waves > 1 || (in.geo.unroll > 2 && ctx->opts.tuning[1] == 0);
        if (can_retry) ctx->jit->reject(plan->cg.source, ctx->jit->last_scratch);   // superseded below: it does not stay in the cache
        if (in.geo.min_waves > 2) {
            in.geo.min_waves--;
        } else if (in.geo.unroll > 2 && ctx->opts.tuning[1] == 0) {
            in.geo.unroll /= 2;            // a smaller sub-tile rather than one wave per SIMD
            if (!in.dense) in.geo.subs_per_chunk *= 2;
            in.geo.min_waves = 3;
        } else if (in.geo.min_waves > 1) {
            in.geo.min_waves--;
        } else {
            break;
        }
    }
}

}  // namespace

namespace qe {

int device_cus(int device) {
    int cus = 0;
    QE_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    return cus > 0 ? cus : 256;
}

void fill_inputs(FusedParams &p, const qe_batch *batch, const Plan &plan) {
    std::memset(&p, 0, sizeof p);
    for (size_t s = 0; s < plan.cg.used_cols.size(); s++) {
        const Column &c = batch->cols[plan.cg.used_cols[s]];
        p.col[s] = c.data;
        p.colvalid[s] = (const unsigned long long *)c.validity;
    }
    p.nrows = batch->nrows;
    // plan constant lookup tables (string ranks / code remaps) ride in the unused tail of col[]
    if (plan.aux_dev.size() != plan.cg.aux_tables.size()) {
        for (const std::vector<int32_t> &t : plan.cg.aux_tables) {
            void *d = nullptr;
            QE_HIP(hipMalloc(&d, std::max<size_t>(t.size() * 4, 16)));
            plan.aux_dev.push_back(d);
            if (!t.empty()) QE_HIP(hipMemcpy(d, t.data(), t.size() * 4, hipMemcpyHostToDevice));
        }
    }
    for (size_t k = 0; k < plan.aux_dev.size(); k++) p.col[kMaxCols - 1 - k] = plan.aux_dev[k];
}

void launch_fused(qe_ctx *ctx, const Plan &plan, FusedParams &p, int grid, bool timed) {
    void *args[] = {&p};
    timed = timed || ctx->opts.profile;
    if (timed) QE_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    QE_HIP(hipModuleLaunchKernel(plan.kernel.fn, grid, 1, 1, plan.geo.threads, 1, 1, 0, ctx->stream, args, nullptr));
    if (timed) QE_HIP(hipEventRecord(ctx->ev1, ctx->stream));
}

void collect_time(qe_ctx *ctx) {
    if (!ctx->opts.profile) return;
    float ms = 0.f;
    QE_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->last_ms = ms;
    ctx->total_ms += ms;
    ctx->launches++;
}

}  // namespace qe

namespace {

int blocks_per_cu(const qe_ctx *ctx, const Plan &plan) {
    if (ctx->opts.tuning[3] % 100 > 0) return ctx->opts.tuning[3] % 100;
    int nb = 0;
    hipError_t e = hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&nb, plan.kernel.fn, plan.geo.threads, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        nb = 2;
    }
    return std::max(1, std::min(nb, 8));
}

// Pass rate of every conjunct on its own (qe_conj_probe), then the evaluation order that fetches the fewest 128-byte lines.
// Model: a column of w bytes per row, needed where a share d of the rows is still alive, costs w * (1 - (1 - d)^(128 / w)) bytes
// per row (whole lines are fetched); conjuncts are taken as independent; the projections' columns are read at the final
// density whatever the order.  Up to 6 conjuncts: every permutation; more: as written.  Returns {} for "as written".
std::vector<int> choose_conjunct_order(qe_ctx *ctx, const qe_batch *batch, const Plan &plan) {
    const int K = plan.cg.nconj;
    if (K < 2 || K > 6 || (int)plan.cg.conj_cols.size() != K) return {};
    const int64_t n = batch->nrows, sub_rows = plan.geo.sub_rows();
    const int64_t full_subs = n / sub_rows;
    const int64_t S = std::min<int64_t>(256, full_subs);
    if (S < 16) return {};
    hipFunction_t f_probe = nullptr;
    QE_HIP(hipModuleGetFunction(&f_probe, plan.kernel.module, "qe_conj_probe"));
    PoolScratch scratch(ctx);
    uint32_t *d_cnt = (uint32_t *)scratch.alloc(64 * 4);
    FusedParams pp;
    fill_inputs(pp, batch, plan);
    pp.nchunks = S;
    pp.stagger_rows = (full_subs / S) * sub_rows;
    pp.blk = (unsigned long long *)d_cnt;
    void *args[] = {&pp};
    const int waves = plan.geo.threads / 64;
    QE_HIP(hipMemsetAsync(d_cnt, 0, 64 * 4, ctx->stream));
    QE_HIP(hipModuleLaunchKernel(f_probe, (unsigned)((S + waves - 1) / waves), 1, 1, plan.geo.threads, 1, 1, 0, ctx->stream, args, nullptr));
    uint32_t h[64];
    QE_HIP(hipMemcpyAsync(h, d_cnt, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<double> rate((size_t)K);
    for (int i = 0; i < K; i++) rate[(size_t)i] = (double)h[i] / (double)(S * sub_rows);
    auto lines = [](double d, int w) { return w <= 0 ? 0.0 : (double)w * (1.0 - std::pow(1.0 - std::min(1.0, std::max(0.0, d)), 128.0 / (double)w)); };
    const size_t ncols = plan.cg.col_width.size();
    auto cost_of = [&](const std::vector<int> &perm) {
        std::vector<char> loaded(ncols, 0);
        double alive = 1.0, cost = 0.0;
        for (int k : perm) {
            for (int c : plan.cg.conj_cols[(size_t)k])
                if (!loaded[(size_t)c]) { loaded[(size_t)c] = 1; cost += lines(alive, plan.cg.col_width[(size_t)c]); }
            alive *= rate[(size_t)k];
        }
        return cost;   // (+ the projection-only columns at the final density: the same for every order)
    };
    std::vector<int> perm((size_t)K), best;
    for (int i = 0; i < K; i++) perm[(size_t)i] = i;
    const std::vector<int> identity = perm;
    const double written = cost_of(identity);
    double best_cost = written;
    do {
        const double c = cost_of(perm);
        if (c < best_cost - 1e-9) { best_cost = c; best = perm; }
    } while (std::next_permutation(perm.begin(), perm.end()));
    // a different order must save at least 3 % of the filter's bytes: otherwise the written order stays (one kernel fewer to build)
    if (best.empty() || best_cost > 0.97 * written) return {};
    return best;
}


// ---- the filter+project executor ---------------------------------------------------------------------------
// run_fused reads top to bottom: plan, conjunct order, geometry candidate, outputs, form, run, bookkeeping, pack.

// The control-block protocol every form shares: zero d_ctrl on the stream, `launch` (what the form enqueues), read the block
// back into h_ctrl, synchronise, account the time.  Returns the block as 32-bit words: [1] = the kernel's error flag;
// ctx->h_ctrl[1] is the kept-row total.
template <typename Launch>
const unsigned int *with_ctrl_block(qe_ctx *ctx, Launch &&launch) {
    QE_HIP(hipMemsetAsync(ctx->d_ctrl, 0, 96, ctx->stream));
    launch();
    QE_HIP(hipMemcpyAsync(ctx->h_ctrl, ctx->d_ctrl, 96, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    collect_time(ctx);
    return (const unsigned int *)ctx->h_ctrl;
}

// diagnostic build (kDbgTrace): per chunk / tile {t_ticket, t_published, t_resolved, t_stored} in 10 ns ticks; nullptr without the bit
unsigned long long *alloc_trace(qe_ctx *ctx, PoolScratch &scratch, int64_t nchunks) {
    if (!debug_bit(ctx, kDbgTrace)) return nullptr;
    void *trace = scratch.alloc((size_t)nchunks * 32);
    QE_HIP(hipMemsetAsync(trace, 0, (size_t)nchunks * 32, ctx->stream));
    return (unsigned long long *)trace;
}

void dump_trace_file(const unsigned long long *d_trace, int64_t nchunks) {
    const char *path = d_trace ? std::getenv("QE_TRACE_FILE") : nullptr;
    if (!path) return;
    std::vector<unsigned long long> tr((size_t)nchunks * 4);
    QE_HIP(hipMemcpy(tr.data(), d_trace, tr.size() * 8, hipMemcpyDeviceToHost));
    if (FILE *f = std::fopen(path, "wb")) {
        std::fwrite(tr.data(), 8, tr.size(), f);
        std::fclose(f);
    }
}

// what the four forms share
struct FusedRun {
    qe_ctx *ctx;
    const qe_batch *batch;
    const Plan &plan;    // at the geometry candidate of this execution
    FusedParams p;       // inputs and outputs filled in
    qe_result *res;
    int64_t cap;         // rows the output columns hold
};

// staging of compacted rows: `rows` rows of every output column (BOOLEAN values and validity as bytes)
void alloc_staging(const FusedRun &r, PoolScratch &scratch, FusedParams &p, size_t rows) {
    for (size_t i = 0; i < r.res->cols.size(); i++) {
        const OutColumn &oc = r.res->cols[i];
        const size_t w = oc.type == QE_BOOLEAN ? 1 : type_width(oc.type);
        p.stage[i] = scratch.alloc(rows * w);
        if (oc.nullable) p.stagevalid[i] = (unsigned char *)scratch.alloc(rows);
    }
}

// The geometry candidate of this execution ("measure, don't guess"): which sub-tile geometry is faster depends on the plan's
// shape (cfg 2: the wide one by 5-8 %; cfg 3: the default by 25 %), so on a large batch the first executions of a plan time
// the candidates in turn (record_geometry_timing) and the fastest one is kept.  Same rows, same order either way.
struct GeoPick {
    qe_ctx::GeoChoice *choice = nullptr;   // null: this plan takes no part in the choice
    int cand = 0;
    std::shared_ptr<Plan> plan;            // the plan at candidate `cand`
    bool exploring() const { return choice && choice->chosen < 0; }
};

// `obase`: the plan in the chosen conjunct order, default geometry -- what the memories hang on; `ordered`: its request
GeoPick pick_geometry_candidate(qe_ctx *ctx, const qe_batch *batch, const PlanRequest &ordered, const std::shared_ptr<Plan> &obase) {
    GeoPick pick;
    pick.plan = obase;
    const int64_t n = batch->nrows;
    const int k2 = obase->geo.unroll > 0 ? (obase->est_regs - 54) / (2 * obase->geo.unroll) : 99;   // registers per row pair
    const bool eligible = !obase->explicit_geometry && obase->est_regs > 0 && n >= (32ll << 20) &&   // (a plain projection too: 6.5 vs 7.3 ms)
                          32 * k2 + 54 <= 256 && !debug_bit(ctx, kDbgNoGeometryChoice);
    if (!eligible) return pick;
    const bool fresh = ctx->geo_choice.find(obase.get()) == ctx->geo_choice.end();
    qe_ctx::GeoChoice *choice = pick.choice = &ctx->geo_choice[obase.get()];
    if (fresh) {   // a decision measured earlier (another context / process) is kept: same plan => same geometry
        // ... unless the two candidates were closer than the box-to-box spread of one binary (+-7 %) when
        // it was measured: such a decision is measured again once per context, on THIS box
        double margin = 1.0;
        const int saved = ctx->jit->load_choice(obase->cg.source, &margin);
        if (saved >= 0 && margin >= 0.07) { choice->chosen = saved; choice->from_cache = true; }
    }
    // exploring: the candidates alternate, kGeoRuns timed executions each, best time wins
    int cand = choice->chosen;
    if (cand < 0) {   // the candidate with the fewest runs so far
        cand = 0;
        for (int c = 1; c < qe_ctx::GeoChoice::kCands; c++)
            if (choice->runs[c] < choice->runs[cand]) cand = c;
    }
    if (cand >= 1) {
        try {
            PlanRequest rq = ordered;
            rq.geo_cand = cand;
            pick.plan = get_plan(ctx, batch, rq);
        } catch (const Error &) {   // this candidate does not build for this plan: it is out of the race
            choice->runs[cand] = 1 << 20;
            if (choice->chosen == cand) choice->chosen = 0;
            cand = 0;
            pick.plan = obase;
        }
    }
    pick.cand = cand;
    return pick;
}

// kGeoRuns timed executions per candidate (best of), then the faster geometry is kept for this plan
void record_geometry_timing(qe_ctx *ctx, const GeoPick &pick, const Plan &obase, int64_t n) {
    constexpr int kGeoRuns = 3;   // one sample each was not reproducible: box / allocation noise is +-7 %, the gap 5-9 %
    qe_ctx::GeoChoice *choice = pick.choice;
    float ms = 0.f;
    QE_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    choice->best_ms[pick.cand] = std::min(choice->best_ms[pick.cand], ms);
    choice->runs[pick.cand]++;
    bool all_done = true;
    for (int c = 0; c < qe_ctx::GeoChoice::kCands; c++) all_done = all_done && choice->runs[c] >= kGeoRuns;
    if (!all_done) return;
    // another geometry must beat the default by a margin (2 %): ties go to the default, which holds fewer registers
    int best = 0;
    for (int c = 1; c < qe_ctx::GeoChoice::kCands; c++)
        if (choice->best_ms[c] < 0.98f * choice->best_ms[0] && (best == 0 || choice->best_ms[c] < choice->best_ms[best])) best = c;
    choice->chosen = best;
    char note[200];
    std::snprintf(note, sizeof note, "default %.4f ms, wide %.4f ms, mid %.4f ms (best of %d each, %lld rows)", choice->best_ms[0],
                  choice->best_ms[1], choice->best_ms[2], kGeoRuns, (long long)n);
    ctx->jit->store_choice(obase.cg.source, choice->chosen, note);
}

// The FIRST execution of a plan knows nothing about its selectivity (a ring kernel that keeps every row costs 12 ms per
// 1 B rows where the dense form needs 6.3): estimate it from 256 chunks spread evenly over the batch -- the count pass
// of the two-pass form over ~4 M rows, filter columns only, a few tens of microseconds.  -1: the batch has no whole chunk.
double sample_selectivity(const FusedRun &r) {
    qe_ctx *ctx = r.ctx;
    const int64_t chunk_rows = r.plan.geo.chunk_rows();
    const int64_t full_chunks = r.batch->nrows / chunk_rows;
    const int64_t S = std::min<int64_t>(256, full_chunks);
    if (S <= 0) return -1.0;
    const int waves = r.plan.geo.threads / 64;
    hipFunction_t f_count = nullptr;
    QE_HIP(hipModuleGetFunction(&f_count, r.plan.kernel.module, "qe_fp_count"));
    PoolScratch scratch(ctx);
    uint32_t *d_sample = (uint32_t *)scratch.alloc((size_t)S * 4);
    FusedParams ps = r.p;
    ps.nchunks = S;
    ps.stagger_chunks = full_chunks / S;
    ps.blk = (unsigned long long *)d_sample;
    void *sargs[] = {&ps};
    QE_HIP(hipModuleLaunchKernel(f_count, (unsigned)((S + waves - 1) / waves), 1, 1, r.plan.geo.threads, 1, 1, 0, ctx->stream, sargs, nullptr));
    std::vector<uint32_t> h((size_t)S);
    QE_HIP(hipMemcpyAsync(h.data(), d_sample, (size_t)S * 4, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    unsigned long long kept = 0;
    for (uint32_t v : h) kept += v;
    return (double)kept / (double)(S * chunk_rows);
}

// The forms of a filter+project execution, chosen from the selectivity the plan showed last time:
//   Dense    chunk == sub-tile, outputs wait in the registers during a blocking look-back and go straight to their final
//            position -- one read of every input, one write of every kept row at ANY selectivity; from kDenseFromSelectivity
//   TwoPass  count the kept rows per chunk, scan, then stream again and store every kept row straight at its final position;
//            superseded by the dense form (kept behind kDbgForceTwoPass)
//   Local    plans that keep a few per cent of their rows at most: per-chunk slots, a scan over the counts, one move
//   Ring     everything else: the single-pass kernel with look-back and LDS rings
enum class Form { Local, Dense, TwoPass, Ring };

struct FormSwitches {   // the force / never bits of qe_options.tuning[5] and the two thresholds the environment may move
    bool force_two_pass, never_two_pass, force_dense, never_dense, force_local, never_local;
    double dense_from, local_upto;
};

FormSwitches form_switches(const qe_ctx *ctx) {
    FormSwitches s;
    s.force_two_pass = debug_bit(ctx, kDbgForceTwoPass);
    s.never_two_pass = debug_bit(ctx, kDbgNeverTwoPass);
    s.force_dense = debug_bit(ctx, kDbgForceDense);
    s.never_dense = debug_bit(ctx, kDbgNeverDense);
    s.dense_from = std::getenv("QE_DENSE_FROM") ? std::atof(std::getenv("QE_DENSE_FROM")) : kDenseFromSelectivity;
    s.force_local = debug_bit(ctx, kDbgForceLocal);
    s.never_local = debug_bit(ctx, kDbgNeverLocal);
    s.local_upto = std::getenv("QE_LOCAL_UPTO") ? std::atof(std::getenv("QE_LOCAL_UPTO")) : kLocalUpToSelectivity;
    return s;
}

// `cg`: the plan's flags; `sel`: the selectivity the plan showed last time (< 0: none yet); `local_overflowed`: see Plan
Form choose_form(const CodegenOutput &cg, double sel, bool local_overflowed, int64_t n, const FormSwitches &s) {
    const bool dense = cg.has_filter && !s.never_dense && !s.force_two_pass && (s.force_dense || sel >= s.dense_from);
    if (dense) return Form::Dense;
    const bool two_pass = cg.has_filter && cg.two_pass && !s.never_two_pass && n < (1ll << 32) &&
                          (s.force_two_pass || sel >= 0.6);   // measured crossover on cfg 2: 0.55 - 0.6
    if (two_pass) return Form::TwoPass;
    const bool local = cg.has_filter && cg.two_pass && !s.never_local && !local_overflowed &&
                       (s.force_local || (n >= kSampleFromRows && sel >= 0 && sel <= s.local_upto));
    return local ? Form::Local : Form::Ring;
}

constexpr int64_t kLocalDeclined = -1, kLocalOverflowed = -2;

// LOCAL form (round 3): for plans that keep a few per cent of their rows at most.  The scan has no inter-wave dependency --
// no ticket, no descriptor, no look-back: every wave parks the kept rows of its (statically strided) chunks in per-chunk
// slots of ring_entries rows; a scan over the per-chunk counts and ONE move kernel put them at their final place.  The
// chunk is sized from the selectivity `sel` the plan showed so that it keeps ~ring_entries / 4 rows.  Returns the kept rows,
// kLocalDeclined (nothing was launched: the move's offsets are 32-bit) or kLocalOverflowed (a chunk kept more rows than its
// slot holds: this plan's rows are not spread evenly); in both cases the caller runs the ring form in this execution.
int64_t run_local(const FusedRun &r, double sel) {
    qe_ctx *ctx = r.ctx;
    const Plan &plan = r.plan;
    const int64_t n = r.batch->nrows;
    const int64_t sub_rows = plan.geo.sub_rows(), ring = plan.cg.fl_ring;
    // expected kept rows per chunk = slot / fill: 2.5 leaves 1.5 slots of head room over the mean (a binomial count of ~200
    // has a standard deviation of ~14); larger chunks were measured faster (cfg 3: 2 Ki rows 2.07 ms, 8 Ki rows 1.71 ms)
    static const double fill = std::getenv("QE_LOCAL_FILL") ? std::atof(std::getenv("QE_LOCAL_FILL")) : 2.5;
    int64_t subs = sel > 0 ? (int64_t)((double)ring / (fill * sel) / (double)sub_rows) : 32;
    if (sel < 0) subs = 1;                               // nothing known (forced): the smallest chunk
    subs = std::max<int64_t>(1, std::min<int64_t>(subs, 32));
    if (ctx->opts.tuning[4] % 10000 > 0) subs = ctx->opts.tuning[4] % 10000;   // explicit sub-tiles per chunk (measurement)
    const int64_t crow = subs * sub_rows;
    const int64_t nchunks = (n + crow - 1) / crow;
    if (nchunks * ring >= (1ll << 32)) return kLocalDeclined;    // 32-bit offsets of the move
    const int waves = plan.geo.threads / 64;
    hipFunction_t f_scan = nullptr, f_move = nullptr;
    QE_HIP(hipModuleGetFunction(&f_scan, plan.kernel.module, "qe_fl_scan"));
    QE_HIP(hipModuleGetFunction(&f_move, plan.kernel.module, "qe_fl_move"));
    PoolScratch scratch(ctx);
    uint32_t *d_counts = (uint32_t *)scratch.alloc((size_t)nchunks * 4);
    uint32_t *d_offsets = (uint32_t *)scratch.alloc((size_t)nchunks * 4);
    uint32_t *d_sums = (uint32_t *)scratch.alloc((size_t)scan_blocks(nchunks) * 4);
    FusedParams lp = r.p;
    alloc_staging(r, scratch, lp, (size_t)nchunks * (size_t)ring);
    lp.capacity = r.cap;
    lp.nchunks = nchunks;
    lp.stagger_rows = crow;
    lp.blk = (unsigned long long *)d_counts;
    lp.l1 = (unsigned long long *)d_offsets;
    lp.error = ctx->d_ctrl + 1;
    lp.total = (unsigned long long *)(ctx->d_ctrl + 2);
    // 20 waves per CU: measured on cfg 3 (600 M rows) 12 / 16 / 20 / 24 waves per CU = 1.99 / 1.85 / 1.78 / 1.85 ms, on cfg 4
    // 0.665 / 0.654 / 0.661 / 0.670 ms -- past 20 the extra streams cost more than the extra loads in flight bring
    int occ = 0;   // of qe_fl_scan itself (it has its own register allocation: no occupancy request, so that it never spills)
    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&occ, f_scan, plan.geo.threads, 0) != hipSuccess) {
        (void)hipGetLastError();
        occ = 2;
    }
    occ = std::max(1, std::min(occ, 8));
    const int bpc = ctx->opts.tuning[3] % 100 > 0 ? ctx->opts.tuning[3] % 100 : std::min(occ, std::max(1, 20 / waves));
    const int64_t max_grid = (int64_t)device_cus(ctx->device) * bpc;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((nchunks + waves - 1) / waves, max_grid));
    const int mgrid = (int)std::max<int64_t>(1, std::min<int64_t>((nchunks + 3) / 4, (int64_t)device_cus(ctx->device) * 8));
    void *largs[] = {&lp};
    const unsigned int *hc = with_ctrl_block(ctx, [&] {
        if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        QE_HIP(hipModuleLaunchKernel(f_scan, grid, 1, 1, plan.geo.threads, 1, 1, 0, ctx->stream, largs, nullptr));
        exclusive_scan<uint32_t>(ctx->stream, ArrayLoad<uint32_t>{d_counts}, d_offsets, d_sums, nchunks, lp.total);
        QE_HIP(hipModuleLaunchKernel(f_move, mgrid, 1, 1, 256, 1, 1, 0, ctx->stream, largs, nullptr));
        if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    });
    if (hc[1] == 5) return kLocalOverflowed;
    if (hc[1] != 0) fail(QE_ERR_INTERNAL, "local form: unexpected error flag");
    return (int64_t)ctx->h_ctrl[1];
}

// DENSE single-pass form (round 2): `dplan` is the plan's dense kernel (its own column slots / aux tables)
int64_t run_dense(const FusedRun &r, const Plan &dplan) {
    qe_ctx *ctx = r.ctx;
    const int64_t n = r.batch->nrows;
    // a tile = the sub-tiles of one workgroup's waves; descriptors are per TILE
    const int waves = dplan.geo.threads / 64;
    const int64_t tile_rows = (int64_t)dplan.geo.sub_rows() * waves;
    const int64_t nchunks = (n + tile_rows - 1) / tile_rows;
    if (nchunks >= (1ll << 31)) fail(QE_ERR_UNSUPPORTED, "batch too large for 32-bit tile tickets");
    const int64_t max_grid = (int64_t)device_cus(ctx->device) * blocks_per_cu(ctx, dplan);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nchunks, max_grid));
    const int64_t nblocks = (nchunks + 63) / 64;
    const size_t desc_words = (size_t)nchunks + 2 * (size_t)nblocks;
    PoolScratch desc_scratch(ctx), trace_scratch(ctx);   // (two: the trace goes back to the pool before the descriptors)
    unsigned long long *desc = (unsigned long long *)desc_scratch.alloc(desc_words * 8);
    FusedParams dp = r.p;                       // same inputs and outputs
    fill_inputs(dp, r.batch, dplan);
    for (size_t i = 0; i < r.res->cols.size(); i++) { dp.out[i] = r.p.out[i]; dp.outvalid[i] = r.p.outvalid[i]; }
    dp.capacity = r.cap;
    dp.desc = desc;
    dp.l1 = desc + nchunks;
    dp.blk = desc + nchunks + nblocks;
    dp.ticket = ctx->d_ctrl;
    dp.error = ctx->d_ctrl + 1;
    dp.total = (unsigned long long *)(ctx->d_ctrl + 2);
    dp.nchunks = nchunks;
    dp.trace = alloc_trace(ctx, trace_scratch, nchunks);
    const unsigned int *hc = with_ctrl_block(ctx, [&] {
        QE_HIP(hipMemsetAsync(desc, 0, desc_words * 8, ctx->stream));
        launch_fused(ctx, dplan, dp, grid);
    });
    dump_trace_file(dp.trace, nchunks);
    if (hc[1] != 0)
        fail(QE_ERR_INTERNAL, hc[1] == 2 ? "dense kernel: ticket grant never posted (spin limit)"
                                         : "dense kernel: look-back spin limit reached (chunk descriptor never published)");
    return (int64_t)ctx->h_ctrl[1];
}

// Two-pass form for HIGH selectivity: no look-back, no LDS ring, no staging round trip (which costs 48 B per kept row
// instead of 16 once the ring overflows)
int64_t run_two_pass(const FusedRun &r) {
    qe_ctx *ctx = r.ctx;
    const Plan &plan = r.plan;
    const int64_t n = r.batch->nrows;
    const int64_t chunk_rows = plan.geo.chunk_rows();
    const int waves = plan.geo.threads / 64;
    const int64_t nchunks = (n + chunk_rows - 1) / chunk_rows;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((nchunks + waves - 1) / waves, (int64_t)device_cus(ctx->device) * 8));
    hipFunction_t f_count = nullptr, f_write = nullptr;
    QE_HIP(hipModuleGetFunction(&f_count, plan.kernel.module, "qe_fp_count"));
    QE_HIP(hipModuleGetFunction(&f_write, plan.kernel.module, "qe_fp_write"));
    PoolScratch scratch(ctx);
    uint32_t *d_counts = (uint32_t *)scratch.alloc((size_t)nchunks * 4);
    FusedParams p = r.p;
    p.capacity = r.cap;
    p.nchunks = nchunks;
    p.blk = (unsigned long long *)d_counts;
    p.error = ctx->d_ctrl + 1;
    p.total = (unsigned long long *)(ctx->d_ctrl + 2);
    void *args[] = {&p};
    with_ctrl_block(ctx, [&] {
        if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev0, ctx->stream));
        QE_HIP(hipModuleLaunchKernel(f_count, grid, 1, 1, plan.geo.threads, 1, 1, 0, ctx->stream, args, nullptr));
        launch_carry_scan<uint32_t, 256>(ctx->stream, d_counts, nchunks, 1, p.total);   // counts -> exclusive offsets, *total = kept rows
        QE_HIP(hipModuleLaunchKernel(f_write, grid, 1, 1, plan.geo.threads, 1, 1, 0, ctx->stream, args, nullptr));
        if (ctx->opts.profile) QE_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    });
    return (int64_t)ctx->h_ctrl[1];
}

// chunks of the ring form: the first `stagger_chunks` chunks (one per resident wave) have graded sizes ((7c mod 16)+1)/16
// of a chunk and cover `stagger_rows` rows; whole chunks follow
struct RingChunks {
    int64_t nchunks = 0, stagger_chunks = 0, stagger_rows = 0;
};
RingChunks ring_chunks(int64_t n, int64_t chunk_rows, int64_t stagger_chunks) {
    RingChunks rc;
    const int64_t sixteenth = chunk_rows / 16;
    // whole periods of 16 chunks cover 136 sixteenths
    const int64_t periods = std::min<int64_t>(stagger_chunks / 16, n / (136 * sixteenth));
    int64_t c = periods * 16, rows = periods * 136 * sixteenth;
    while (c < stagger_chunks && rows < n) {
        rows += (((7 * c) & 15) + 1) * sixteenth;
        c++;
    }
    rc.stagger_rows = rows;
    if (rows >= n) {
        rc.nchunks = rc.stagger_chunks = c;        // every chunk is a staggered one
    } else {
        rc.stagger_chunks = stagger_chunks;
        rc.nchunks = stagger_chunks + (n - rows + chunk_rows - 1) / chunk_rows;
    }
    return rc;
}

// RING form: the single-pass kernel (ticket per chunk, look-back over the chunk descriptors, kept rows wait in per-wave LDS
// rings).  `pick` is timed while the geometry choice of `obase` is still exploring.
int64_t run_ring(const FusedRun &r, const GeoPick &pick, const Plan &obase) {
    qe_ctx *ctx = r.ctx;
    const Plan &plan = r.plan;
    const int64_t n = r.batch->nrows;
    const int64_t chunk_rows = plan.geo.chunk_rows();
    const int waves = plan.geo.threads / 64;
    const int64_t max_grid = (int64_t)device_cus(ctx->device) * blocks_per_cu(ctx, plan);
    const RingChunks rc = ring_chunks(n, chunk_rows, plan.geo.stagger ? max_grid * waves : 0);
    const int64_t nchunks = rc.nchunks;
    if (nchunks >= (1ll << 31)) fail(QE_ERR_UNSUPPORTED, "batch too large for 32-bit chunk tickets");
    const int grid = (int)std::min<int64_t>((nchunks + waves - 1) / waves, max_grid);
    static const bool dbg_grid = std::getenv("QE_DEBUG_GRID") != nullptr;
    if (dbg_grid) std::fprintf(stderr, "[qe] ring kernel: grid %d x %d threads (%d blocks per CU), unroll %d, %d sub-tiles per chunk, ring %d, min_waves %d\n",
                               grid, plan.geo.threads, blocks_per_cu(ctx, plan), plan.geo.unroll, plan.geo.subs_per_chunk, plan.geo.ring_entries, plan.geo.min_waves);
    // scratch: look-back descriptors + one staging slot (chunk_rows rows per output column) per resident wave
    PoolScratch scratch(ctx);
    // descriptors: [nchunks] level 0, then [nblocks] level 1, then [nblocks] block counters -- one allocation,
    // zeroed by ONE memset on the stream before every launch
    const int64_t nblocks = (nchunks + 63) / 64;
    const size_t desc_words = (size_t)nchunks + 2 * (size_t)nblocks;
    unsigned long long *desc = (unsigned long long *)scratch.alloc(desc_words * 8);
    FusedParams p = r.p;
    if (plan.cg.has_filter) {
        const size_t slots = (size_t)grid * waves * plan.geo.nbuf;   // one staging (overflow) slot per LDS buffer
        alloc_staging(r, scratch, p, slots * (size_t)plan.geo.slot_rows());
    }
    p.capacity = r.cap;
    p.desc = desc;
    p.l1 = desc + nchunks;
    p.blk = desc + nchunks + nblocks;
    p.ticket = ctx->d_ctrl;
    p.error = ctx->d_ctrl + 1;
    p.total = (unsigned long long *)(ctx->d_ctrl + 2);
    p.nchunks = nchunks;
    p.stagger_chunks = rc.stagger_chunks;
    p.stagger_rows = rc.stagger_rows;
    p.stats = (unsigned long long *)(ctx->d_ctrl + 16);   // bytes 64..95 of the control block
    p.trace = alloc_trace(ctx, scratch, nchunks);
    // flags, tickets and descriptors are re-zeroed on the stream before EVERY launch
    const unsigned int *hc = with_ctrl_block(ctx, [&] {
        QE_HIP(hipMemsetAsync(desc, 0, desc_words * 8, ctx->stream));
        launch_fused(ctx, plan, p, grid, pick.exploring());
    });
    if (pick.exploring()) record_geometry_timing(ctx, pick, obase, n);
    dump_trace_file(p.trace, nchunks);
    if (debug_bit(ctx, kDbgWaitStats))
        std::fprintf(stderr, "[qe stats] chunks %llu failed_tries %llu forced_waits %llu blocking_spins %llu\n", ctx->h_ctrl[11],
                     ctx->h_ctrl[8], ctx->h_ctrl[10], ctx->h_ctrl[9]);
    if (hc[1] != 0) fail(QE_ERR_INTERNAL, "fused kernel: look-back spin limit reached (tile descriptor never published)");
    return (int64_t)ctx->h_ctrl[1];
}

// output columns of `plan`, sized for `cap` rows (BOOLEAN values and validity as bytes until pack_byte_columns), into res and p
void alloc_outputs(qe_ctx *ctx, const Plan &plan, qe_result *res, int64_t cap, FusedParams &p) {
    for (size_t i = 0; i < res->cols.size(); i++) {
        OutColumn &oc = res->cols[i];
        if (oc.type == QE_BOOLEAN) {
            oc.bytes_data = ctx->pool.alloc((size_t)cap);
            p.out[i] = oc.bytes_data;
        } else {
            oc.data = ctx->pool.alloc(type_width(oc.type) * (size_t)cap);
            p.out[i] = oc.data;
        }
        if (oc.nullable) {
            oc.bytes_valid = (uint8_t *)ctx->pool.alloc((size_t)cap);
            p.outvalid[i] = oc.bytes_valid;
        }
    }
}

// nullable / boolean outputs were written one byte per row: pack them into bitmaps
void pack_byte_columns(qe_ctx *ctx, qe_result *res) {
    bool packed = false;
    for (OutColumn &oc : res->cols) {
        if (oc.type == QE_BOOLEAN) {
            oc.data = ctx->pool.alloc(bitmap_bytes(res->count));
            launch_pack_bytes(ctx->stream, (const uint8_t *)oc.bytes_data, res->count, (uint64_t *)oc.data);
            packed = true;
        }
        if (oc.nullable) {
            oc.validity = (uint64_t *)ctx->pool.alloc(bitmap_bytes(res->count));
            launch_pack_bytes(ctx->stream, oc.bytes_valid, res->count, oc.validity);
            packed = true;
        }
    }
    if (!packed) return;
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    for (OutColumn &oc : res->cols) {
        ctx->pool.release(oc.bytes_data);
        ctx->pool.release(oc.bytes_valid);
        oc.bytes_data = nullptr;
        oc.bytes_valid = nullptr;
    }
}

qe_result *run_fused(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter, const qe_expr *const *projs,
                     int32_t nproj) {
    const PlanRequest written{filter, projs, nproj};
    const std::shared_ptr<Plan> base = get_plan(ctx, batch, written);   // as written, default geometry: selectivity and order hang on it
    const int64_t n = batch->nrows;
    // Conjunct order (round 3): the load stages follow the evaluation order of the filter's AND chain.  As written,
    // `c < 0.5 AND a < 100` reads c in full and a for half of the rows; evaluated as `a < 100 AND c < 0.5` it reads a in full, c
    // where a passes.  On its first execution on a large batch a plan measures the pass rate of every conjunct on its own
    // (qe_conj_probe over 256 sub-tiles spread over the batch), the host picks the order that fetches the fewest 128-byte
    // lines, and the plan keeps it.  Same rows, same order: a row is kept iff every conjunct is TRUE.
    if (base->cg.has_probe && !base->conj_decided && n >= kSampleFromRows && !debug_bit(ctx, kDbgWrittenConjunctOrder)) {
        base->conj_decided = true;
        base->conj_order = choose_conjunct_order(ctx, batch, *base);
    }
    const std::vector<int> order = base->conj_order;
    PlanRequest ordered = written;
    if (!order.empty()) ordered.conj_order = &order;
    const std::shared_ptr<Plan> obase = order.empty() ? base : get_plan(ctx, batch, ordered);
    const GeoPick pick = pick_geometry_candidate(ctx, batch, ordered, obase);
    const Plan &plan = *pick.plan;

    ResultPtr res = new_result(ctx, 0);   // (the count is known after the scan)
    const int64_t cap = ctx->opts.result_capacity_rows > 0 ? std::min<int64_t>(ctx->opts.result_capacity_rows, n) : n;
    res->capacity = cap;
    for (const OutSpec &os : plan.cg.outs) {
        OutColumn oc;
        oc.type = os.type;
        oc.nullable = os.nullable;
        oc.dict = os.dict;
        oc.dict_handle.d = os.dict;
        res->cols.push_back(oc);
    }
    if (n == 0) return res.release();
    FusedRun run{ctx, batch, plan, {}, res.get(), cap};
    fill_inputs(run.p, batch, plan);
    alloc_outputs(ctx, plan, res.get(), cap, run.p);

    const FormSwitches sw = form_switches(ctx);
    if (plan.cg.has_filter && plan.cg.two_pass && base->last_selectivity < 0 && !sw.force_dense && !sw.never_dense && !sw.force_two_pass &&
        n >= kSampleFromRows && !debug_bit(ctx, kDbgNoSelectivitySample))
        base->last_selectivity = sample_selectivity(run);
    Form form = choose_form(plan.cg, base->last_selectivity, base->local_overflowed, n, sw);
    int64_t total = 0;
    if (form == Form::Local) {
        total = run_local(run, base->last_selectivity);
        if (total == kLocalOverflowed) base->local_overflowed = true;   // .. and the plan stays with the single-pass kernel
        if (total < 0) form = Form::Ring;
    }
    if (form == Form::Dense) {
        PlanRequest rq = written;
        rq.dense = true;
        total = run_dense(run, *get_plan(ctx, batch, rq));
    } else if (form == Form::TwoPass) {
        total = run_two_pass(run);
    } else if (form == Form::Ring) {
        total = run_ring(run, pick, *obase);
    }

    ctx->last_form = !plan.cg.has_filter ? QE_FORM_NO_FILTER
                     : form == Form::Local ? QE_FORM_LOCAL : form == Form::Dense ? QE_FORM_DENSE : form == Form::TwoPass ? QE_FORM_TWO_PASS : QE_FORM_RING;
    pick.plan->last_selectivity = base->last_selectivity = (double)total / (double)n;
    if (total > cap)
        fail(QE_ERR_INVALID_ARG, "result has " + std::to_string(total) + " rows but result_capacity_rows is " +
                                     std::to_string(cap));
    res->count = total;
    pack_byte_columns(ctx, res.get());
    return res.release();
}

}  // namespace

// ---- internals of the overlapped scan + exchange (qe_comm.cpp: qe_filter_project_gather) ---------------------------------
// kept rows of every slice of `slice_rows` rows (a multiple of the plan's chunk) of the batch: ONE launch of the count pass
// (qe_fp_count: the filter's columns only, late materialisation included) and a 4-byte read-back per chunk
std::vector<int64_t> qe_int_count_slices(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter, const qe_expr *const *projs, int32_t nproj,
                                  int64_t *slice_rows_io, int32_t nslices) {
    const int64_t n = batch->nrows;
    auto plan = get_plan(ctx, batch, PlanRequest{filter, projs, nproj});
    const int64_t chunk_rows = plan->geo.chunk_rows();
    int64_t slice_rows = (n + nslices - 1) / std::max(1, nslices);
    slice_rows = std::max<int64_t>(chunk_rows, (slice_rows + chunk_rows - 1) / chunk_rows * chunk_rows);
    *slice_rows_io = slice_rows;
    const int64_t ns = n > 0 ? (n + slice_rows - 1) / slice_rows : 0;
    std::vector<int64_t> counts((size_t)ns, 0);
    if (n == 0) return counts;
    if (!filter || !plan->cg.two_pass) {   // no Filter node: every row is kept
        for (int64_t k = 0; k < ns; k++) counts[(size_t)k] = std::min(slice_rows, n - k * slice_rows);
        return counts;
    }
    const int64_t nchunks = (n + chunk_rows - 1) / chunk_rows;
    const int waves = plan->geo.threads / 64;
    hipFunction_t f_count = nullptr;
    QE_HIP(hipModuleGetFunction(&f_count, plan->kernel.module, "qe_fp_count"));
    PoolScratch scratch(ctx);
    uint32_t *d_counts = (uint32_t *)scratch.alloc((size_t)nchunks * 4);
    FusedParams p;
    fill_inputs(p, batch, *plan);
    p.nchunks = nchunks;
    p.blk = (unsigned long long *)d_counts;
    void *args[] = {&p};
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((nchunks + waves - 1) / waves, (int64_t)device_cus(ctx->device) * 8));
    QE_HIP(hipModuleLaunchKernel(f_count, grid, 1, 1, plan->geo.threads, 1, 1, 0, ctx->stream, args, nullptr));
    std::vector<uint32_t> h((size_t)nchunks);
    QE_HIP(hipMemcpyAsync(h.data(), d_counts, (size_t)nchunks * 4, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t per = slice_rows / chunk_rows;
    for (int64_t c = 0; c < nchunks; c++) counts[(size_t)(c / per)] += h[(size_t)c];
    return counts;
}

// Projection(Filter(Scan)) over rows [row_begin, row_begin + nrows) of the batch (row_begin a multiple of 64: bitmap words do
// not straddle the cut): a view of the batch's columns, no copy
qe_result *qe_int_run_fused_slice(qe_ctx *ctx, const qe_batch *batch, int64_t row_begin, int64_t nrows, const qe_expr *filter,
                           const qe_expr *const *projs, int32_t nproj) {
    if (row_begin % 64 != 0 || row_begin < 0 || nrows < 0 || row_begin + nrows > batch->nrows) fail(QE_ERR_INTERNAL, "bad slice");
    qe_batch view;
    view.nrows = nrows;
    for (const Column &c : batch->cols) {
        Column v = c;
        v.owned = false;
        if (c.data) v.data = (char *)c.data + (c.type == QE_BOOLEAN ? (size_t)(row_begin / 64) * 8 : type_width(c.type) * (size_t)row_begin);
        if (c.validity) v.validity = c.validity + row_begin / 64;
        view.cols.push_back(v);
    }
    return run_fused(ctx, &view, filter, projs, nproj);
}

extern "C" {

int32_t qe_filter_project(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                          const qe_expr *const *projections, int32_t nproj, qe_result **out) {
    if (!ctx || !batch || !out) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(ctx, [&] {
        need_device(ctx);
        if (batch->schema_only) fail(QE_ERR_INVALID_ARG, "schema-only batch (qe_batch_describe) cannot be executed");
        if (ctx->opts.exec_mode == QE_EXEC_PER_NODE) {
            *out = run_per_node(ctx, batch, filter, projections, nproj);
            ctx->last_form = QE_FORM_PER_NODE;
        } else
            *out = run_fused(ctx, batch, filter, projections, nproj);
    });
}

int32_t qe_filter_project_prepare(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                  const qe_expr *const *projections, int32_t nproj) {
    if (!ctx || !batch) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        if (ctx->device >= 0) need_device(ctx);
        if (ctx->opts.exec_mode == QE_EXEC_FUSED) {
            PlanRequest rq{filter, projections, nproj};
            rq.load = ctx->device >= 0;
            auto pl = get_plan(ctx, batch, rq);
            // the second geometry candidate (qe_ctx::geo_choice) is compiled ahead of time as well, so that the choice on
            // the device never waits for the JIT
            const int k2 = pl->geo.unroll > 0 ? (pl->est_regs - 54) / (2 * pl->geo.unroll) : 99;
            if (!pl->explicit_geometry && pl->est_regs > 0 && 32 * k2 + 54 <= 256 && !debug_bit(ctx, kDbgNoGeometryChoice))
                for (int c = 1; c < qe_ctx::GeoChoice::kCands; c++)
                    try {
                        PlanRequest cand = rq;
                        cand.geo_cand = c;
                        (void)get_plan(ctx, batch, cand);
                    } catch (const Error &) {   // optional candidates: the default plan above is what prepare guarantees
                    }
            // the dense single-pass kernel (plans that keep a large share of their rows) is compiled ahead of time as well
            if (filter && !debug_bit(ctx, kDbgNeverDense)) {
                rq.dense = true;
                (void)get_plan(ctx, batch, rq);
            }
        }
    });
}

int32_t qe_filter_project_source(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                 const qe_expr *const *projections, int32_t nproj, const char **out) {
    if (!ctx || !batch || !out) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        PlanRequest rq{filter, projections, nproj};
        rq.dense = filter && debug_bit(ctx, kDbgForceDense);   // a context forced into the dense form shows that kernel
        rq.load = false;
        auto plan = get_plan(ctx, batch, rq);
        ctx->source_scratch = plan->cg.source;
        *out = ctx->source_scratch.c_str();
    });
}

int32_t qe_filter_project_geometry(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                   const qe_expr *const *projections, int32_t nproj, int32_t *out_chosen, int32_t *out_from_cache) {
    if (!ctx || !batch || !out_chosen) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        PlanRequest rq{filter, projections, nproj};
        rq.load = false;
        auto plan = get_plan(ctx, batch, rq);
        if (!plan->conj_order.empty()) {   // the geometry memory belongs to the plan in its chosen conjunct order
            rq.conj_order = &plan->conj_order;
            plan = get_plan(ctx, batch, rq);
        }
        *out_chosen = -1;
        if (out_from_cache) *out_from_cache = 0;
        auto it = ctx->geo_choice.find(plan.get());
        if (it != ctx->geo_choice.end()) {
            *out_chosen = it->second.chosen;
            if (out_from_cache) *out_from_cache = it->second.from_cache ? 1 : 0;
        } else {
            double margin = 1.0;
            const int saved = ctx->jit->load_choice(plan->cg.source, &margin);
            if (saved >= 0 && margin >= 0.07) {   // (a closer call is measured again by the next execution on this context)
                *out_chosen = saved;
                if (out_from_cache) *out_from_cache = 1;
            }
        }
    });
}

int32_t qe_filter_project_conjunct_order(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                         const qe_expr *const *projections, int32_t nproj, int32_t *out_order, int32_t capacity,
                                         int32_t *out_nconj) {
    if (!ctx || !batch || !out_nconj || capacity < 0 || (capacity > 0 && !out_order)) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        PlanRequest rq{filter, projections, nproj};
        rq.load = false;
        auto plan = get_plan(ctx, batch, rq);
        const int K = plan->cg.nconj;
        *out_nconj = plan->conj_decided ? K : -1;
        for (int i = 0; i < K && i < capacity; i++) out_order[i] = plan->conj_order.empty() ? i : plan->conj_order[(size_t)i];
    });
}

}  // extern "C"
