// qe_setop.cpp -- host side of UNION / INTERSECT / EXCEPT [ALL] over two results (kernels: qe_setop.hip): the
// dictionaries of the STRING columns are settled on the host, the two sides are concatenated with the placement code of
// qe_result_concat, and every form but UNION ALL sorts the concatenation by all its columns with the ORDER BY driver, marks the
// tuple starts with the window operator's boundary flags, decides per sorted position whether its row is kept, and gathers
// the kept rows with the row gather every operator uses.
#include <algorithm>

#include "qe_exec.h"
#include "qe_kernels.h"
#include "qe_scan.h"

namespace qe {

MergedDict merge_dictionaries(const DictData &left, const DictData &right) {
    MergedDict md;
    md.dict = std::make_shared<DictData>();
    md.dict->entries = left.entries;
    md.dict->index = left.index;
    md.table.resize(right.entries.size());
    for (size_t i = 0; i < md.table.size(); i++) {
        const std::string &s = right.entries[i];
        const int32_t found = left.find(s);
        if (found >= 0) {
            md.table[i] = found;
            continue;
        }
        md.table[i] = (int32_t)md.dict->entries.size();
        md.dict->index.emplace(s, md.table[i]);   // first occurrence wins
        md.dict->entries.push_back(s);
    }
    return md;
}

namespace {

constexpr int kMaxSortedCols = 8, kMaxConcatCols = 16;   // the sort's keys; the limit of qe_result_concat
constexpr int64_t kMaxRows = (1ll << 32) - 2;            // rows are uint32 with one sentinel, as in the join

bool is_nullable(const OutColumn &c) { return c.nullable || c.validity != nullptr; }

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

    // ---- 1. the dictionaries: compare by string, not by code.  One object on both sides: the codes as they are; else the
    // left entries, then the right entries the left does not hold, and a table right code -> merged code ----
    PoolScratch sc(ctx);
    std::vector<std::shared_ptr<DictData>> merged((size_t)ncols);
    std::vector<std::vector<int32_t>> tables;   // the host copies, alive until the uploads have completed
    std::vector<const int *> d_table((size_t)ncols, nullptr);
    uint32_t translated_mask = 0, any_validity = 0;
    tables.reserve((size_t)ncols);
    for (int32_t c = 0; c < ncols; c++) {
        const OutColumn &l = left->cols[(size_t)c], &r = right->cols[(size_t)c];
        if (is_nullable(l) || is_nullable(r)) any_validity |= 1u << c;
        if (l.type != QE_STRING || l.dict.get() == r.dict.get()) continue;
        MergedDict md = merge_dictionaries(*l.dict, *r.dict);
        std::shared_ptr<DictData> m = std::move(md.dict);
        std::vector<int32_t> table = std::move(md.table);
        int *d = (int *)sc.alloc(table.size() * 4);
        tables.push_back(std::move(table));
        if (!tables.back().empty())
            QE_HIP(hipMemcpyAsync(d, tables.back().data(), tables.back().size() * 4, hipMemcpyHostToDevice, ctx->stream));
        d_table[(size_t)c] = d;
        merged[(size_t)c] = std::move(m);
        translated_mask |= 1u << c;
    }
    int64_t stats[4] = {nl, nr, 0, (int64_t)__builtin_popcount(translated_mask)};

    // ---- 2. the concatenated source: left rows, then right rows ----
    ResultPtr cat = concat_output(ctx, left, n, any_validity);
    for (int32_t c = 0; c < ncols; c++)
        if (merged[(size_t)c]) cat->cols[(size_t)c].dict = cat->cols[(size_t)c].dict_handle.d = merged[(size_t)c];
    concat_place(ctx, sc, left, 0, cat.get(), 0);
    concat_place(ctx, sc, right, nl, cat.get(), translated_mask);
    for (int32_t c = 0; c < ncols; c++)
        if (d_table[(size_t)c])
            launch_setop_translate_codes(ctx->stream, (const int *)right->cols[(size_t)c].data, nr, d_table[(size_t)c],
                                         (int)right->cols[(size_t)c].dict->entries.size(), (int *)cat->cols[(size_t)c].data + nl);
    QE_HIP(hipGetLastError());
    if (!sorts || n == 0) {   // UNION ALL is the concatenation; of no rows at all every form is
        QE_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < 4; i++) ctx->set_stats[i] = stats[i];
        return cat.release();
    }

    // ---- 3. the sort by every column, and the tuple starts through the same row ids ----
    std::vector<qe_sort_key> keys;
    for (int32_t c = 0; c < ncols; c++) keys.push_back({c, 0});
    SortDriver drv{ctx, sc, cat.get(), keys.data(), ncols};
    drv.prepare();
    RadixBuffers rb(sc, n);
    drv.sort(rb, true);
    const uint32_t *perm = rb.sorted_rows();
    const int64_t nwords = bitmap_words(n);
    unsigned long long *pstart = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    unsigned long long *peer = (unsigned long long *)sc.alloc(bitmap_bytes(n));   // equals pstart: every key is a partition key
    unsigned long long *d_count = (unsigned long long *)sc.alloc(16);
    uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(nwords + 1) * 4);
    uint32_t *pstart_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
    WinFlagArgs fa{};
    fa.nkeys = fa.npart = ncols;
    fa.n = n;
    fa.pstart = pstart;
    fa.peer = peer;
    fa.npartitions = d_count;
    fa.perm = perm;
    for (int32_t c = 0; c < ncols; c++) {
        const OutColumn &kc = cat->cols[(size_t)c];
        fa.type[c] = kc.type;
        fa.data[c] = kc.data;
        fa.validity[c] = (const unsigned long long *)kc.validity;
        fa.ranks[c] = drv.d_ranks[(size_t)c];
        fa.nranks[c] = drv.nranks[(size_t)c];
    }
    QE_HIP(hipMemsetAsync(d_count, 0, 16, ctx->stream));
    launch_win_flags(ctx->stream, fa);
    bitmap_ranks(ctx->stream, (const uint64_t *)pstart, nullptr, n, pstart_prefix, sums, nullptr);
    unsigned long long h_count = 0;
    QE_HIP(hipMemcpyAsync(&h_count, d_count, 8, hipMemcpyDeviceToHost, ctx->stream));   // G: joins the sort's own read-backs
    QE_HIP(hipGetLastError());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t G = (int64_t)h_count;
    if (G < 1 || G > n) fail(QE_ERR_INTERNAL, std::string(who) + ": " + std::to_string(G) + " tuples of " + std::to_string(n) + " rows");
    stats[2] = G;

    // ---- 4. the kept rows ----
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

    // ---- 5. kept sorted positions -> source rows -> the output ----
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
    for (int i = 0; i < 4; i++) ctx->set_stats[i] = stats[i];
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

int32_t qe_ctx_last_set_stats(const qe_ctx *ctx, int64_t out[4]) {
    if (!ctx || !out) return QE_ERR_INVALID_ARG;
    for (int i = 0; i < 4; i++) out[i] = ctx->set_stats[i];
    return QE_OK;
}

}  // extern "C"
