// qe_join.cpp -- host side of the hash equi-join (kernels: qe_join.hip) and qe_batch_from_result, the way a
// result goes into the next plan without leaving HBM.
#include <algorithm>
#include <cstdlib>
#include <functional>

#include "qe_exec.h"
#include "qe_scan.h"

namespace qe {
namespace {

constexpr int64_t kMaxSideRows = (1ll << 32) - 2;   // rows are uint32 with one sentinel
constexpr int kMaxDirBits = 26;                     // 64 Mi buckets: the directory stays at 256 MiB

// one side of a join, whichever of the two it is: columns (nullable: those with a bitmap) and a row count
using SideCol = SourceColumn;
struct Side {
    int64_t nrows = 0;
    std::vector<SideCol> cols;
};

Side side_of(const qe_join_input *in, const char *who) {
    if (!in || (in->result != nullptr) == (in->batch != nullptr))
        fail(QE_ERR_INVALID_ARG, std::string(who) + ": exactly one of qe_join_input.result and .batch must be set");
    Side s;
    if (in->result) {
        s.nrows = in->result->count;
        for (const OutColumn &c : in->result->cols) s.cols.push_back({c.type, c.data, c.validity, c.dict, c.validity != nullptr});
    } else {
        if (in->batch->schema_only) fail(QE_ERR_INVALID_ARG, std::string(who) + ": a schema-only batch has no rows to join");
        s.nrows = in->batch->nrows;
        for (const Column &c : in->batch->cols) s.cols.push_back({c.type, c.data, c.validity, c.dict, c.validity != nullptr});
    }
    for (const SideCol &c : s.cols)
        if (c.type == QE_STRING && !c.dict) fail(QE_ERR_INVALID_ARG, std::string(who) + ": STRING column without dictionary");
    return s;
}

void check_cols(const Side &s, const int32_t *cols, int32_t n, const char *who, const char *what) {
    if (n < 0 || (n > 0 && !cols)) fail(QE_ERR_INVALID_ARG, std::string(who) + ": bad " + what + " list");
    check_columns(who, what, cols, n, s.cols.size());
}

uint64_t hash_mask_from_env() {
    // test switch: keep only the low n bits of the hash, so that many keys share one
    if (const char *e = std::getenv("QE_JOIN_HASH_BITS")) {
        const int n = std::atoi(e);
        if (n >= 0 && n < 64) return n == 0 ? 0ull : (~0ull >> (64 - n));
    }
    return ~0ull;
}

}  // namespace
}  // namespace qe

struct qe_join_table {
    qe::Side build;                 // the build input's columns (read again by the gathers of a probe) + its dictionaries
    std::vector<int32_t> key_cols;
    int64_t m = 0;                  // build rows with a key
    int dbits = 4;
    uint64_t mask = ~0ull;
    uint32_t *dir = nullptr;        // 2^dbits + 1 bucket offsets
    uint32_t *rows = nullptr;       // build row per sorted entry
    unsigned long long *img[4] = {nullptr, nullptr, nullptr, nullptr};   // key images per sorted entry
};

namespace qe {
namespace {

void free_table(qe_ctx *ctx, qe_join_table *t) {
    if (!t) return;
    ctx->pool.release(t->dir);
    ctx->pool.release(t->rows);
    for (auto *p : t->img) ctx->pool.release(p);
    delete t;
}

// key columns of `side` as the kernels read them.  STRING keys go through a code -> canonical BUILD code table made here
// from the two dictionaries (-1: the build dictionary does not hold the string; a dictionary that lists a string twice
// maps both codes to the first): `tables` keeps the host copies alive until the uploads have completed.
JoinKeyCols key_columns(qe_ctx *ctx, PoolScratch &sc, const Side &side, const int32_t *cols, int32_t nkeys, const Side &build,
                        const std::vector<int32_t> &build_cols, std::vector<std::vector<int32_t>> &tables) {
    JoinKeyCols kc{};
    kc.nkeys = nkeys;
    tables.reserve((size_t)nkeys);
    for (int32_t k = 0; k < nkeys; k++) {
        const SideCol &c = side.cols[(size_t)cols[k]];
        kc.type[k] = c.type;
        kc.data[k] = c.data;
        kc.validity[k] = (const unsigned long long *)c.validity;
        if (c.type != QE_STRING) continue;
        const DictData &bd = *build.cols[(size_t)build_cols[(size_t)k]].dict;
        kc.ncodes[k] = (int)c.dict->entries.size();
        if (c.dict.get() == &bd && bd.index.size() == bd.entries.size()) continue;   // the build dictionary itself, no duplicates: codes as they are
        std::vector<int32_t> table(c.dict->entries.size());
        for (size_t i = 0; i < table.size(); i++) table[i] = bd.find(c.dict->entries[i]);
        int *d = (int *)sc.alloc(table.size() * 4);
        tables.push_back(std::move(table));
        if (!tables.back().empty())
            QE_HIP(hipMemcpyAsync(d, tables.back().data(), tables.back().size() * 4, hipMemcpyHostToDevice, ctx->stream));
        kc.remap[k] = d;
    }
    return kc;
}

qe_join_table *build_table(qe_ctx *ctx, const qe_join_input *in, const int32_t *key_cols, int32_t nkeys) {
    const char *who = "qe_join_build";
    Side side = side_of(in, who);
    if (nkeys < 1 || nkeys > 4 || !key_cols) fail(QE_ERR_INVALID_ARG, std::string(who) + ": 1 <= nkeys <= 4");
    check_cols(side, key_cols, nkeys, who, "key");
    if (side.nrows > kMaxSideRows) fail(QE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 2 rows");
    need_device(ctx);

    std::unique_ptr<qe_join_table, std::function<void(qe_join_table *)>> t(new qe_join_table(), [ctx](qe_join_table *p) { free_table(ctx, p); });
    t->build = std::move(side);
    t->key_cols.assign(key_cols, key_cols + nkeys);
    t->mask = hash_mask_from_env();
    const int64_t n = t->build.nrows;

    PoolScratch sc(ctx);
    std::vector<std::vector<int32_t>> tables;
    JoinBuildArgs ba{};
    ba.kc = key_columns(ctx, sc, t->build, key_cols, nkeys, t->build, t->key_cols, tables);
    ba.n = n;
    ba.mask = t->mask;
    RadixBuffers rb(sc, n);
    unsigned long long *img[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < nkeys; k++) img[k] = ba.img[k] = (unsigned long long *)sc.alloc((size_t)n * 8);
    ba.hash = rb.keys[0];
    ba.rows = rb.rows[0];
    ba.valid_words = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    ba.nvalid = (unsigned long long *)sc.alloc(16);
    QE_HIP(hipMemsetAsync(ba.nvalid, 0, 16, ctx->stream));
    launch_join_build_keys(ctx->stream, ba);
    unsigned long long m = 0;
    QE_HIP(hipMemcpyAsync(&m, ba.nvalid, 8, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));   // (also: the code tables are on the device now)
    if ((int64_t)m > n) fail(QE_ERR_INTERNAL, std::string(who) + ": counted more keyed rows than rows");
    t->m = (int64_t)m;

    // directory over the top hash bits: about one bucket per keyed row
    int dbits = 4;
    while (dbits < kMaxDirBits && (1ll << dbits) < t->m) dbits++;
    t->dbits = dbits;

    // stable LSD radix sort of (hash, row) on the digits that cover the directory bits; then the rows without a key go
    // behind the others (one pass on their bit).  Entries with equal hashes (so: equal keys) stay in build-row order.
    if (n > 0) {
        const int ndigits = (dbits + 3) / 4;
        for (int shift = 64 - 4 * ndigits; shift < 64; shift += 4) rb.pass(ctx->stream, shift);
        if (t->m < n) rb.pass(ctx->stream, 65, (const uint64_t *)ba.valid_words);
    }
    t->dir = (uint32_t *)ctx->pool.alloc(((size_t)1 << dbits) * 4 + 16);
    launch_join_directory(ctx->stream, rb.sorted_keys(), t->m, dbits, t->dir);
    t->rows = (uint32_t *)ctx->pool.alloc((size_t)t->m * 4);
    if (t->m > 0) QE_HIP(hipMemcpyAsync(t->rows, rb.sorted_rows(), (size_t)t->m * 4, hipMemcpyDeviceToDevice, ctx->stream));
    for (int k = 0; k < nkeys; k++) {
        t->img[k] = (unsigned long long *)ctx->pool.alloc((size_t)t->m * 8);
        launch_gather_rows(ctx->stream, 8, img[k], rb.sorted_rows(), t->m, t->img[k]);
    }
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    ctx->join_stats.store(t->m, 0, 0, 0);
    return t.release();
}

qe_result *probe_table(qe_ctx *ctx, const qe_join_table *t, const qe_join_input *in, const int32_t *key_cols, int32_t nkeys, int32_t join_type,
                       const int32_t *probe_out, int32_t nprobe_out, const int32_t *build_out, int32_t nbuild_out) {
    const char *who = "qe_join_probe";
    const Side side = side_of(in, who);
    if (!key_cols || nkeys != (int32_t)t->key_cols.size()) fail(QE_ERR_INVALID_ARG, std::string(who) + ": nkeys differs from the table's");
    const bool outer = join_type == QE_JOIN_RIGHT || join_type == QE_JOIN_FULL;
    if ((join_type < QE_JOIN_INNER || join_type > QE_JOIN_ANTI) && !outer) fail(QE_ERR_INVALID_ARG, std::string(who) + ": unknown join type");
    check_cols(side, key_cols, nkeys, who, "key");
    for (int32_t k = 0; k < nkeys; k++)
        if (side.cols[(size_t)key_cols[k]].type != t->build.cols[(size_t)t->key_cols[(size_t)k]].type)
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": key column " + std::to_string(k) + " is " + type_name(side.cols[(size_t)key_cols[k]].type) +
                                         " on the probe side and " + type_name(t->build.cols[(size_t)t->key_cols[(size_t)k]].type) + " on the build side");
    check_cols(side, probe_out, nprobe_out, who, "probe output");
    check_cols(t->build, build_out, nbuild_out, who, "build output");
    const int32_t head_type = join_type == QE_JOIN_RIGHT ? QE_JOIN_INNER : join_type == QE_JOIN_FULL ? QE_JOIN_LEFT : join_type;   // the HEAD's
    const bool pairs = head_type == QE_JOIN_INNER || head_type == QE_JOIN_LEFT;
    if (!pairs && nbuild_out != 0) fail(QE_ERR_INVALID_ARG, std::string(who) + ": a SEMI / ANTI join has no build columns");
    if (nprobe_out + nbuild_out < 1) fail(QE_ERR_INVALID_ARG, std::string(who) + ": no output column");
    if (side.nrows > kMaxSideRows) fail(QE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 2 rows");
    need_device(ctx);

    const int64_t n = side.nrows, nbuild = t->build.nrows;
    PoolScratch sc(ctx);
    std::vector<std::vector<int32_t>> tables;
    JoinProbeArgs pa{};
    pa.kc = key_columns(ctx, sc, side, key_cols, nkeys, t->build, t->key_cols, tables);
    pa.t.dir = t->dir;
    pa.t.rows = t->rows;
    for (int k = 0; k < 4; k++) pa.t.img[k] = t->img[k];
    pa.t.dbits = t->dbits;
    pa.t.nkeys = nkeys;
    pa.t.mask = t->mask;
    pa.n = n;
    pa.join_type = head_type;
    const int64_t nblocks = join_probe_blocks(n);
    pa.cnt = (uint32_t *)sc.alloc((size_t)n * 4);
    if (pairs) pa.first = (uint32_t *)sc.alloc((size_t)n * 4);
    pa.blocksum = (unsigned long long *)sc.alloc((size_t)nblocks * 8);
    unsigned long long *d_ctl = (unsigned long long *)sc.alloc(32);   // [0] total, [1] longest walk (u32), [2] tail rows (RIGHT / FULL)
    pa.longest = (uint32_t *)(d_ctl + 1);
    QE_HIP(hipMemsetAsync(d_ctl, 0, 32, ctx->stream));
    uint32_t *tail_prefix = nullptr;
    if (outer && nbuild > 0) {   // the marks belong to this call: the table is not written
        pa.matched = (unsigned long long *)sc.alloc(bitmap_bytes(nbuild));
        QE_HIP(hipMemsetAsync(pa.matched, 0, bitmap_bytes(nbuild), ctx->stream));
    }
    launch_join_count(ctx->stream, pa);
    launch_carry_scan<unsigned long long, 1024>(ctx->stream, pa.blocksum, nblocks, 1, d_ctl);   // 64-bit: the pairs may pass 2^32
    if (pa.matched) {   // matched -> unmatched, and its ranks: the tail's length arrives with the head's
        const int64_t nwords = bitmap_words(nbuild);
        tail_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
        uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(nwords + 1) * 4);
        launch_join_unmatched(ctx->stream, pa.matched, nbuild);
        bitmap_ranks(ctx->stream, (const uint64_t *)pa.matched, nullptr, nbuild, tail_prefix, sums, d_ctl + 2);
    }
    unsigned long long h_ctl[4] = {0, 0, 0, 0};
    QE_HIP(hipMemcpyAsync(h_ctl, d_ctl, 32, hipMemcpyDeviceToHost, ctx->stream));   // the one read-back: the output's size
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t total = (int64_t)h_ctl[0];   // at most 2^32 rows of at most 2^32 matches: fits; an output too large for the
                                               // device is reported by the pool below (QE_ERR_OOM)
    const int64_t tail = (int64_t)h_ctl[2];
    if (tail < 0 || tail > nbuild) fail(QE_ERR_INTERNAL, std::string(who) + ": " + std::to_string(tail) + " unmatched of " + std::to_string(nbuild) + " build rows");
    const int64_t nout = total + tail;

    ResultPtr res = new_result(ctx, nout);
    pa.total = (unsigned long long)total;
    pa.prow_out = (uint32_t *)sc.alloc((size_t)nout * 4);
    if (pairs) pa.brow_out = (uint32_t *)sc.alloc((size_t)nout * 4);
    launch_join_write(ctx->stream, pa);
    if (tail > 0) {   // the tail extends the two lists: no probe row, the unmatched build rows ascending
        QE_HIP(hipMemsetAsync(pa.prow_out + total, 0xFF, (size_t)tail * 4, ctx->stream));
        bitmap_positions(ctx->stream, (const uint64_t *)pa.matched, nullptr, nbuild, tail_prefix, pa.brow_out + total, tail, false);
    }

    emit_joined(ctx, res.get(), nout, side.cols, probe_out, nprobe_out, pa.prow_out, t->build.cols, build_out, nbuild_out, pa.brow_out, outer,
                head_type == QE_JOIN_LEFT, kGatherBlocksWide);   // (no launch for no rows: launch_gather_rows returns at once, as before)
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    ctx->join_stats.store(t->m, n, nout, (int64_t)(uint32_t)h_ctl[1]);
    if (outer) ctx->outer_stats.store(1, total, tail, nbuild - tail);
    return res.release();
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int32_t qe_join_build(qe_ctx *ctx, const qe_join_input *build, const int32_t *key_cols, int32_t nkeys, qe_join_table **out) {
    if (out) *out = nullptr;
    if (!ctx || !build || !key_cols || !out) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] { *out = build_table(ctx, build, key_cols, nkeys); });
}

int64_t qe_join_table_rows(const qe_join_table *table) { return table ? table->m : -1; }

void qe_join_table_free(qe_ctx *ctx, qe_join_table *table) {
    if (!ctx || !table) return;
    free_table(ctx, table);
}

int32_t qe_join_probe(qe_ctx *ctx, const qe_join_table *table, const qe_join_input *probe, const int32_t *key_cols, int32_t nkeys, int32_t join_type,
                      const int32_t *probe_out_cols, int32_t nprobe_out, const int32_t *build_out_cols, int32_t nbuild_out, qe_result **out) {
    if (out) *out = nullptr;
    if (!ctx || !table || !probe || !key_cols || !out) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        *out = probe_table(ctx, table, probe, key_cols, nkeys, join_type, probe_out_cols, nprobe_out, build_out_cols, nbuild_out);
    });
}

int32_t qe_ctx_last_join_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::join_stats, out); }

int32_t qe_ctx_last_outer_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::outer_stats, out); }

int32_t qe_batch_from_result(qe_ctx *ctx, const qe_result *result, qe_batch **out) {
    if (out) *out = nullptr;
    if (!ctx || !result || !out) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        std::unique_ptr<qe_batch> b(new qe_batch());
        b->nrows = result->count;
        for (const OutColumn &c : result->cols) {
            Column col;
            col.type = c.type;
            col.data = c.data;
            col.validity = c.validity;
            col.dict = c.dict;
            col.owned = false;
            b->cols.push_back(col);
        }
        // the batch reads the result's buffers: a qe_result_free that comes before the batch's is deferred (free_batch)
        b->view_of = const_cast<qe_result *>(result);
        b->view_of->views++;
        *out = b.release();
    });
}

}  // extern "C"
