// qe_exec.h -- what the files behind the C ABI share (not part of the ABI, not exported from libqe_hip.so):
//   qe_context.cpp   errors, pools, contexts, dictionaries, batches, expression handles, stream calibrations
//   qe_api.cpp       plan cache + geometry (get_plan), the filter+project executor and its entry points
//   qe_groupby.cpp   the global aggregate and the GROUP BY routes with their entry points: launches and uploads
//   qe_group_finish.h / .cpp   what the accumulator words of a group mean and how they become result columns (host only, no HIP;
//                    exported, like qe_expr_rules.h, so that a test program can link it)
//   qe_result.cpp    results on the device: how every operator builds one (new_result, add_column, gather_columns), and
//                    their way to the host
//   qe_sort.cpp      ORDER BY with top-k, the stable multi-key radix sort (RadixBuffers, SortDriver) that the join build and
//                    the device group finish share with it, and that sort with the boundary flags of its runs (SortedRuns):
//                    how the four sorted-run operators below begin
//   qe_comm.cpp      the RCCL exchange step, the concatenation of results, and the two-sided concatenation with merged
//                    dictionaries (concat_two_sided) that the set operations, the ASOF join and the range join begin with
//   qe_join.cpp      the hash equi-join of two device-resident sides, a result as the next plan's batch
//   qe_window.cpp    window functions over a result: sorted runs, the row gather, the segmented scans
//   qe_ordered.cpp   ordered-set aggregates per group (quantiles, COUNT DISTINCT, MODE): sorted runs per argument column,
//                    then ranks, compaction and picks over the sorted rows
//   qe_setop.cpp     UNION / INTERSECT / EXCEPT [ALL] of two results: the two sides as one, sorted runs over every column,
//                    a keep bitmap from per-tuple counts of the two sides, the row gather
//   qe_two_sided.cpp what the joins of two results share: the checks of their arguments, the key sort of the two sides as
//                    one (TwoSidedKeys: concat_two_sided, sorted runs over (by.., value), the eligible and the right rows), and
//                    the output step (emit_joined)
//   qe_asof.cpp      the ASOF join of two results: one key sort over (by.., on), the nearest eligible right position per
//                    left row, the output step
//   qe_range.cpp     the range join of two results: a key sort over (by.., lo) and one over (by.., hi), two ordinals per left
//                    row, a 64-bit scan of the counts, the load-balanced expansion into row pairs, the output step
//   qe_csv_device.cpp  CSV text parsed on the device: the text sources and their upload, the passes as steps of one driver,
//                    the field packer behind the dictionary and the patch list, one body for both entry points
#pragma once

#include <memory>
#include <new>
#include <string>
#include <vector>

#include "qe_internal.h"
#include "qe_kernels.h"

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
inline int64_t bitmap_words(int64_t n) { return (n + 63) / 64; }
inline size_t bitmap_bytes(int64_t n) { return (size_t)bitmap_words(n) * 8; }
inline size_t column_bytes(int t, int64_t n) { return t == QE_BOOLEAN ? bitmap_bytes(n) : type_width(t) * (size_t)n; }

// ---- qe_result.cpp --------------------------------------------------------------------------------------
void free_result(qe_ctx *ctx, qe_result *r);

// A result under construction: whatever throws on the way, every buffer its columns hold goes back to the context's pool.
struct ResultDeleter {
    qe_ctx *ctx;
    void operator()(qe_result *r) const { free_result(ctx, r); }
};
using ResultPtr = std::unique_ptr<qe_result, ResultDeleter>;
inline ResultPtr own_result(qe_ctx *ctx, qe_result *r) { return ResultPtr(r, ResultDeleter{ctx}); }
// an empty result of `count` rows (capacity = count)
ResultPtr new_result(qe_ctx *ctx, int64_t count);
// One more column of `nrows` rows: values and, if nullable, a validity bitmap from the pool, uninitialised.  The column is
// pushed BEFORE its buffers are allocated, so a failing allocation leaves nothing that the result does not own.
OutColumn &add_column(qe_ctx *ctx, qe_result *res, int type, bool nullable, const std::shared_ptr<DictData> &dict, int64_t nrows);
// the column turned out to hold no NULL: its bitmap goes back to the pool
void drop_validity(qe_ctx *ctx, OutColumn &c);
// dst[j] = row rows[j] of a source column, j < nout.  Row 0xFFFFFFFF ("no row", the LEFT join's) gives a zero value and
// validity 0; a source without bitmap reads as all valid.  dst carries a bitmap exactly when it is nullable.  max_blocks: the
// grid cap of the launches, kGatherBlocks or kGatherBlocksWide (qe_kernels.h)
void gather_column(qe_ctx *ctx, int type, const void *data, const uint64_t *validity, const uint32_t *rows, int64_t nout, OutColumn &dst,
                   int max_blocks);
// the same for every column of src_cols, into the first columns of dst (kGatherBlocks)
void gather_columns(qe_ctx *ctx, const std::vector<OutColumn> &src_cols, const uint32_t *rows, int64_t nout, qe_result *dst);

// ---- qe_sort.cpp: the stable LSD radix sort of (u64 key, u32 row) pairs -----------------------------------
// Its scratch: two key buffers, two row buffers and the histogram words of launch_radix_pass.  The caller fills side 0 --
// its own buffers, when it already holds the keys and rows there -- and runs the passes it needs.
struct RadixBuffers {
    unsigned long long *keys[2];
    uint32_t *rows[2];
    uint32_t *hist;
    int64_t m;
    int cur = 0;
    RadixBuffers(PoolScratch &sc, int64_t m, unsigned long long *keys0 = nullptr, uint32_t *rows0 = nullptr);
    // one stable pass over the 4 key bits at `shift`, or (shift 64 / 65) over the rows' bits in `validity`
    void pass(hipStream_t s, int shift, const uint64_t *validity = nullptr);
    unsigned long long *sorted_keys() const { return keys[cur]; }
    uint32_t *sorted_rows() const { return rows[cur]; }
};

// The stable multi-key sort of a result's rows: ORDER BY, and the partition / order sort of the window operator.
struct SortDriver {
    qe_ctx *ctx;
    PoolScratch &sc;
    const qe_result *src;
    const qe_sort_key *keys;
    int32_t nkeys;
    std::vector<const int *> d_ranks;   // per key: compareTo ranks of a STRING column's dictionary
    std::vector<int> nranks;
    std::vector<std::vector<std::vector<int32_t>>> h_ranks;   // the host tables, alive until the uploads have completed
    unsigned long long *d_bits = nullptr;
    int64_t radix_passes = 0;

    void prepare();
    // images of key k for m elements: of rows 0..m-1 (perm == nullptr; rows_out[i] = i unless null) or of rows perm[0..m)
    void images(int32_t k, int64_t m, const uint32_t *perm, unsigned long long *keys_out, uint32_t *rows_out);
    // bits that differ between the m images (a digit without such a bit is the same in every key: its pass is skipped)
    unsigned long long varying(const unsigned long long *k, int64_t m);
    // stable sort of the row ids in side 0 of `rb` (identity: they are 0..m-1 and are written here) by all keys
    void sort(RadixBuffers &rb, bool identity);
};

// How the window, the ordered-set aggregates, the set operations and the ASOF join begin: the stable sort of src's rows by
// `keys` from the identity, then the boundary flags of the sorted rows (qe_window.hip).  Everything is queued on the context's
// stream and nothing is read back beyond what the sort reads itself (prepare, varying); the caller reads the counter when it
// suits it.  The sort allocates from `ss` alone; the flag buffers are the caller's, so they may outlive `ss`.  The object
// keeps the host rank tables of STRING keys, as SortDriver does: it lives as long as `ss`.
struct SortedRuns {
    SortDriver sorter;
    const uint32_t *rows = nullptr;   // the sorted row ids, in `ss`; null without keys: no sort runs, the rows stay as they are
    SortedRuns(qe_ctx *ctx, PoolScratch &ss, const qe_result *src, const qe_sort_key *keys, int32_t nkeys);
    int64_t radix_passes() const { return sorter.radix_passes; }
    // Zeroes the 16-byte counter, then launch_win_flags (qe_kernels.h) through `rows`: pstart = the starts of the runs of the
    // first npart keys, peer = of all keys, word 0 of the counter = the set bits of pstart.  Bitmaps of bitmap_bytes(src->count).
    void flag(int32_t npart, unsigned long long *pstart, unsigned long long *peer, unsigned long long *counter);
    // prefix[w] = set bits of pstart before word w (bitmap_ranks; sums: its scan_blocks(words + 1) scratch)
    void rank_starts(const unsigned long long *pstart, uint32_t *prefix, uint32_t *sums);
};
// the run count read back: who + ": <count> <noun> of <n> rows" (QE_ERR_INTERNAL) unless 1 <= count <= n
int64_t checked_runs(const char *who, unsigned long long count, const char *noun, int64_t n);

// ---- qe_comm.cpp: the placement code behind qe_result_concat / qe_gather, shared with the set operations and the ASOF join --
// A result of `total` rows with the column types and dictionaries of `like`; bit c of any_validity: column c carries a
// validity bitmap.  BOOLEAN values and validity are zeroed: concat_place ORs segments in.
ResultPtr concat_output(qe_ctx *ctx, const qe_result *like, int64_t total, uint32_t any_validity);
// the rows of `part` at row offset `off` of such a result (bit c of skip_values: the caller writes column c's values itself)
void concat_place(qe_ctx *ctx, PoolScratch &sc, const qe_result *part, int64_t off, qe_result *out, uint32_t skip_values);
// `ncols` columns of `src` as a result that borrows their buffers (never freed): what the two take for a column subset
qe_result column_view(const qe_result *src, const int32_t *cols, int32_t ncols);

constexpr int64_t kMaxRows = (1ll << 32) - 2;   // of a two-sided operator's sides together: rows are uint32 with one sentinel, as in the join
inline bool is_nullable(const OutColumn &c) { return c.nullable || c.validity != nullptr; }
// The merged dictionary of a STRING column whose sides carry different dictionary objects.  dict: the left entries in their
// order, then the right entries the left does not hold, in the right's order; table[right code] = merged code (an entry the
// left holds: the code the left finds for it).
struct MergedDict {
    std::shared_ptr<DictData> dict;
    std::vector<int32_t> table;
};
MergedDict merge_dictionaries(const DictData &left, const DictData &right);
// The two sides of a set operation or an ASOF join as one result of left->count + right->count rows, the left rows from
// row loff on and the right rows from roff on.  The sides agree in their column types (the caller has checked, and that
// every STRING column has a dictionary); a column is nullable when either side is; a STRING column whose sides differ in
// dictionary object gets the merged dictionary and the right side's codes translated into it.  Queued on the context's
// stream: the caller synchronises before it lets go of what this returns.
struct TwoSided {
    ResultPtr cat;
    uint32_t translated = 0;                    // bit c: column c was translated
    std::vector<std::vector<int32_t>> tables;   // the host copies of the translation tables, alive until the uploads have completed
};
TwoSided concat_two_sided(qe_ctx *ctx, PoolScratch &sc, const qe_result *left, int64_t loff, const qe_result *right, int64_t roff);

// ---- qe_two_sided.cpp: what the two-sided joins share (the hash probe, the ASOF join, the range join) ----------------------
// What every join of two results is called with.  `who` is the entry point's name: every message begins with it.
struct TwoSidedCall {
    const char *who;
    const qe_result *left, *right;
    const int32_t *left_by, *right_by;
    int32_t nby;
    const int32_t *left_out, *right_out;
    int32_t nleft_out, nright_out, join_type;
};
constexpr uint32_t kJoinsPairs = 1u << QE_JOIN_INNER | 1u << QE_JOIN_LEFT, kJoinsOuter = 1u << QE_JOIN_RIGHT | 1u << QE_JOIN_FULL,
                   kJoinsAll = kJoinsPairs | 1u << QE_JOIN_SEMI | 1u << QE_JOIN_ANTI | kJoinsOuter;
// What can be said without reading either side (a caller's handle is only touched once this has returned): 0 to 7 by columns
// with both lists there, option_error (the caller's verdict on its own flags, null: none), join_type among join_types (a
// kJoins.. set), the out lists, "no output column", "a SEMI / ANTI join has no right columns".  All QE_ERR_INVALID_ARG.
void check_call(const TwoSidedCall &q, uint32_t join_types, const char *option_error);
// every cols[i] is below ncols, or who + ": <what> column <c> out of range"
void check_columns(const char *who, const char *what, const int32_t *cols, int32_t n, size_t ncols);
// a value column of a join: the side it belongs to, its index there and its name in messages ("left lo", "right on")
struct ValueColumn {
    bool right;
    int32_t col;
    const char *name;
};
// What the sides themselves say: every by, value and out column is in range, the by columns agree in type pairwise and the
// STRING ones have dictionaries, the value columns are DOUBLE, INT64 or INT32 and of one type (all QE_ERR_INVALID_ARG); then
// the rows of both sides together are at most kMaxRows (QE_ERR_UNSUPPORTED).  The caller's need_device comes after it.
void check_sides(const TwoSidedCall &q, const ValueColumn *values, int nvalues);

// The key sort of two sides: the by columns and one value column of each side as one result (concat_two_sided; among equal
// keys the right rows stand first when right_first) and its rows sorted by (by.., value) (SortedRuns); then, by mark(), the
// sorted rows with a whole key (`eligible`) and the right rows among those (`right`) as bitmaps (launch_asof_eligible), and
// the ranks of `right` per word.  Queued on the context's stream.  LIFETIME: the key result and `sc` go back to the pool only
// after the stream has been synchronised -- the caller synchronises before this object or `sc` goes out of scope.
struct TwoSidedKeys {
    int64_t nl, nr, n;
    TwoSided both;                              // both.cat: the key result (its validity pointers are what the kernels read)
    const qe_sort_key keys[8] = {{0, 0}, {1, 0}, {2, 0}, {3, 0}, {4, 0}, {5, 0}, {6, 0}, {7, 0}};   // ascending; the first nby + 1
    SortedRuns runs;
    AsofSides sides;
    unsigned long long *eligible, *right;       // bitmap_bytes(n) each
    uint32_t *sums, *right_prefix;              // scan_blocks(words + 1) words of scan scratch, free again; words + 1 ranks
    TwoSidedKeys(qe_ctx *ctx, PoolScratch &sc, const TwoSidedCall &q, int32_t left_value, int32_t right_value, bool right_first);
    void mark();   // (its own step: the ASOF join flags its partitions between the sort and this, as it always has)
};

// what the row gather reads of a source column, whichever kind of column it is
struct SourceColumn {
    int type;
    const void *data;
    const uint64_t *validity;
    std::shared_ptr<DictData> dict;
    bool nullable;
    SourceColumn(int type, const void *data, const uint64_t *validity, std::shared_ptr<DictData> dict, bool nullable)
        : type(type), data(data), validity(validity), dict(std::move(dict)), nullable(nullable) {}
    SourceColumn(const OutColumn &c) : SourceColumn(c.type, c.data, c.validity, c.dict, is_nullable(c)) {}
};
// one more column of res: src gathered by rows[0..nout) (gather_column: max_blocks); no launch for nout == 0
void emit_column(qe_ctx *ctx, qe_result *res, int64_t nout, const SourceColumn &src, const uint32_t *rows, bool force_nullable, int max_blocks);
// The output step of a join: the listed left columns by lrows (nullable whatever the source when left_nullable: the tail of a
// RIGHT / FULL join), then the listed right columns by rrows (nullable whatever the source when right_nullable: the unmatched
// rows of a LEFT / FULL join), into a result of nout rows.
template <typename L, typename R>
void emit_joined(qe_ctx *ctx, qe_result *res, int64_t nout, const std::vector<L> &lcols, const int32_t *left_out, int32_t nleft_out,
                 const uint32_t *lrows, const std::vector<R> &rcols, const int32_t *right_out, int32_t nright_out, const uint32_t *rrows,
                 bool left_nullable, bool right_nullable, int max_blocks) {
    res->cols.reserve((size_t)(nleft_out + nright_out));
    for (int32_t i = 0; i < nleft_out; i++) emit_column(ctx, res, nout, lcols[(size_t)left_out[i]], lrows, left_nullable, max_blocks);
    for (int32_t i = 0; i < nright_out; i++) emit_column(ctx, res, nout, rcols[(size_t)right_out[i]], rrows, right_nullable, max_blocks);
}

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
