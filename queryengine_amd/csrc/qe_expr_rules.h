// qe_expr_rules.h -- what the two expression evaluators decide on the host at plan time, before either touches a row.
// Gen::emit (qe_codegen.cpp) carries a node out as C text of the fused kernel, Exec::eval (qe_pernode.cpp) as a kernel launch over
// columns and bitmap words.  The rules below do not depend on that: each function RETURNS the decision.  Host only, no HIP.
#pragma once

#include "qe_internal.h"

namespace qe {

inline bool is_arithmetic_fn(int fn) { return fn == QE_FN_ADD || fn == QE_FN_SUB || fn == QE_FN_MUL || fn == QE_FN_DIV || fn == QE_FN_MOD; }
inline bool is_comparison_fn(int fn) { return fn >= QE_FN_CMP_LT && fn <= QE_FN_CMP_NE; }
inline bool is_null_test_fn(int fn) { return fn == QE_FN_IS_NULL || fn == QE_FN_IS_NOT_NULL; }
inline bool cmp_holds(int fn, int c) {   // the comparison `fn` on a compareTo result c
    return fn == QE_FN_CMP_LT ? c < 0 : fn == QE_FN_CMP_LE ? c <= 0 : fn == QE_FN_CMP_GE ? c >= 0 : fn == QE_FN_CMP_GT ? c > 0 : fn == QE_FN_CMP_EQ ? c == 0 : c != 0;
}

// The conjuncts (node ids) of the AND chain at `root`, left to right; a root that is no AND is its only conjunct.
std::vector<int> split_conjuncts(const Expr &e, int root);

// One N_COLUMN node: the batch column and whether its VALUE is read.  The direct operand of a null test is asked for its
// validity only (the fused kernel never loads its values, the per-node executor gathers only its bitmap).
struct ColumnUse { int col; bool value; };
// The column nodes of the subtree at `root` in node order (= left to right), each checked against the batch (col_types[c] =
// type of batch column c): an index out of range or a type other than the expression's raises QE_ERR_PROGRAM.
std::vector<ColumnUse> column_uses(const Expr &e, int root, const std::vector<int> &col_types);

// One operand of a STRING operation: the dictionary its codes index, or a bare literal (exactly one of the two is set).
struct StrSide { const DictData *dict; const std::string *lit; };
// How `a fn b` over STRING operands is carried out; [0] is a's side, [1] is b's.
struct StringCompare {
    // Constant: literal against literal, `value`.  Codes: = / <> on the codes as they are, a literal side compares as lit[side].
    // Ranks: table[side][code] of a dictionary side, lit[side] of a literal side.
    enum Kind { Constant, Codes, Ranks } kind = Constant;
    bool value = false;
    int32_t lit[2] = {0, 0};
    std::vector<int32_t> table[2];
};
StringCompare plan_string_compare(int fn, const StrSide &a, const StrSide &b);

// STRING values of two branches (IF's THEN / ELSE, COALESCE's operands) in ONE dictionary.
struct DictUnion {
    std::shared_ptr<DictData> dict;   // a new dictionary with its own serial number
    bool remap_second = false;        // the second side's codes go through `remap`; all other codes hold as they are
    std::vector<int32_t> remap;       // code in the second side's dictionary -> code in `dict`
    int32_t lit[2] = {0, 0};          // code of a literal side
};
DictUnion unify_dictionaries(const StrSide &first, const StrSide &second);

// a bare string literal as a value: a one-entry dictionary, code 0
std::shared_ptr<DictData> literal_dictionary(const std::string &lit);

// True (and `out` = L) when the numeric literal L is integral with |L| < 2^53: `(double)x OP L` over an integer x can then
// be compared on the integers.
bool exact_integer_literal(double lit, long long &out);

}  // namespace qe
