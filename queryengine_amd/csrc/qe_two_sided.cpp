// qe_two_sided.cpp -- what the joins of two results share (qe_exec.h): the checks of their arguments,
// the key sort of the two sides as one that the ASOF join and the range join begin with, and the output step of all three.
#include "qe_exec.h"
#include "qe_scan.h"

namespace qe {

void check_call(const TwoSidedCall &q, uint32_t join_types, const char *option_error) {
    const std::string who = std::string(q.who) + ": ";
    if (q.nby < 0 || q.nby > 7) fail(QE_ERR_INVALID_ARG, who + "0 to 7 by columns");   // with the value column: the sort's 8 keys
    if (q.nby > 0 && (!q.left_by || !q.right_by)) fail(QE_ERR_INVALID_ARG, who + "by columns missing");
    if (option_error) fail(QE_ERR_INVALID_ARG, who + option_error);
    if (q.join_type < 0 || q.join_type > QE_JOIN_FULL || !((join_types >> q.join_type) & 1u))   // (4 to 7 are in no set)
        fail(QE_ERR_INVALID_ARG, who + (join_types == kJoinsAll ? "unknown join type" : "the join type is INNER or LEFT"));
    if (q.nleft_out < 0 || q.nright_out < 0) fail(QE_ERR_INVALID_ARG, who + "negative column count");
    if ((q.nleft_out > 0 && !q.left_out) || (q.nright_out > 0 && !q.right_out)) fail(QE_ERR_INVALID_ARG, who + "output columns missing");
    if ((int64_t)q.nleft_out + q.nright_out < 1) fail(QE_ERR_INVALID_ARG, who + "no output column");
    if ((q.join_type == QE_JOIN_SEMI || q.join_type == QE_JOIN_ANTI) && q.nright_out != 0)
        fail(QE_ERR_INVALID_ARG, who + "a SEMI / ANTI join has no right columns");
}

void check_columns(const char *who, const char *what, const int32_t *cols, int32_t n, size_t ncols) {
    for (int32_t i = 0; i < n; i++)
        if (cols[i] < 0 || cols[i] >= (int32_t)ncols)
            fail(QE_ERR_INVALID_ARG, std::string(who) + ": " + what + " column " + std::to_string(cols[i]) + " out of range");
}

namespace {

// the value columns are DOUBLE, INT64 or INT32, and all of one type
void check_value_types(const TwoSidedCall &q, const ValueColumn *values, int nvalues) {
    std::string all;
    bool one_type = true;
    for (int i = 0; i < nvalues; i++) {
        const int t = (values[i].right ? q.right : q.left)->cols[(size_t)values[i].col].type;
        if (t != QE_DOUBLE && t != QE_INT64 && t != QE_INT32)
            fail(QE_ERR_INVALID_ARG, std::string(q.who) + ": the " + values[i].name + " column is " + type_name(t) + ", not DOUBLE, INT64 or INT32");
        one_type = one_type && t == (values[0].right ? q.right : q.left)->cols[(size_t)values[0].col].type;
        all += std::string(i == 0 ? "" : i + 1 < nvalues ? ", " : " and ") + type_name(t) + " (" + values[i].name + ")";
    }
    if (!one_type) fail(QE_ERR_INVALID_ARG, std::string(q.who) + ": the value columns are " + all);
}

// the scratch key result, the dictionaries of its STRING by columns settled.  The stable sort keeps the concatenation's order
// inside a run of equal keys, so the side that stands first there stands first among equals
TwoSided concat_keys(qe_ctx *ctx, PoolScratch &sc, const TwoSidedCall &q, int32_t left_value, int32_t right_value, bool right_first) {
    std::vector<int32_t> lkeys(q.left_by, q.left_by + q.nby), rkeys(q.right_by, q.right_by + q.nby);
    lkeys.push_back(left_value);
    rkeys.push_back(right_value);
    const qe_result lview = column_view(q.left, lkeys.data(), q.nby + 1), rview = column_view(q.right, rkeys.data(), q.nby + 1);
    return concat_two_sided(ctx, sc, &lview, right_first ? q.right->count : 0, &rview, right_first ? 0 : q.left->count);
}

}  // namespace

void check_sides(const TwoSidedCall &q, const ValueColumn *values, int nvalues) {
    const size_t nlcols = q.left->cols.size(), nrcols = q.right->cols.size();
    check_columns(q.who, "left by", q.left_by, q.nby, nlcols);
    check_columns(q.who, "right by", q.right_by, q.nby, nrcols);
    for (int i = 0; i < nvalues; i++) check_columns(q.who, values[i].name, &values[i].col, 1, values[i].right ? nrcols : nlcols);
    check_columns(q.who, "left output", q.left_out, q.nleft_out, nlcols);
    check_columns(q.who, "right output", q.right_out, q.nright_out, nrcols);
    for (int32_t k = 0; k < q.nby; k++) {
        const OutColumn &l = q.left->cols[(size_t)q.left_by[k]], &r = q.right->cols[(size_t)q.right_by[k]];
        if (l.type != r.type)
            fail(QE_ERR_INVALID_ARG, std::string(q.who) + ": by column " + std::to_string(k) + " is " + type_name(l.type) + " on the left and " +
                                         type_name(r.type) + " on the right");
        if (l.type == QE_STRING && (!l.dict || !r.dict)) fail(QE_ERR_INVALID_ARG, std::string(q.who) + ": STRING by column without dictionary");
    }
    check_value_types(q, values, nvalues);
    if (q.left->count + q.right->count > kMaxRows) fail(QE_ERR_UNSUPPORTED, std::string(q.who) + ": 2^32 - 1 rows or more");
}

TwoSidedKeys::TwoSidedKeys(qe_ctx *ctx, PoolScratch &sc, const TwoSidedCall &q, int32_t left_value, int32_t right_value, bool right_first)
    : nl(q.left->count), nr(q.right->count), n(nl + nr), both(concat_keys(ctx, sc, q, left_value, right_value, right_first)),
      runs(ctx, sc, both.cat.get(), keys, q.nby + 1) {
    const int64_t nwords = bitmap_words(n);
    eligible = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    right = (unsigned long long *)sc.alloc(bitmap_bytes(n));
    sums = (uint32_t *)sc.alloc((size_t)scan_blocks(nwords + 1) * 4);
    right_prefix = (uint32_t *)sc.alloc((size_t)(nwords + 1) * 4);
    sides = AsofSides{runs.rows, n, right_first ? nr : nl, right_first ? 1 : 0};
}

void TwoSidedKeys::mark() {
    AsofEligibleArgs ea{};
    ea.s = sides;
    ea.nkeys = runs.sorter.nkeys;
    for (int32_t k = 0; k < ea.nkeys; k++) ea.validity[k] = (const unsigned long long *)both.cat->cols[(size_t)k].validity;
    ea.eligible = eligible;
    ea.right = right;
    launch_asof_eligible(runs.sorter.ctx->stream, ea);
    bitmap_ranks(runs.sorter.ctx->stream, (const uint64_t *)right, nullptr, n, right_prefix, sums, nullptr);
}

void emit_column(qe_ctx *ctx, qe_result *res, int64_t nout, const SourceColumn &src, const uint32_t *rows, bool force_nullable, int max_blocks) {
    OutColumn &oc = add_column(ctx, res, src.type, force_nullable || src.nullable, src.dict, nout);
    if (nout > 0) gather_column(ctx, src.type, src.data, src.validity, rows, nout, oc, max_blocks);
}

}  // namespace qe
