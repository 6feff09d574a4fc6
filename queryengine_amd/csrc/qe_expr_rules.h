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
// `validity_only` (optional, per node id): further function nodes that look at the validity of a direct column operand alone --
// an IN / LIKE that plan_member folds to a constant.
std::vector<ColumnUse> column_uses(const Expr &e, int root, const std::vector<int> &col_types, const std::vector<char> *validity_only = nullptr);

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
// The same, and L fits the width of `int_type` (QE_INT64 / QE_INT32): the comparison runs at the integer operand's width.
bool exact_integer_literal(double lit, int int_type, long long &out);
// Node `id` as a cast of an integer expression to DOUBLE, `(double)x` with x INT64 / INT32 and no literal: the node id of x,
// else -1.  A comparison with an exact integer literal and an IN list of them are then carried out on x itself.
int integer_cast_operand(const Expr &e, int id);


// ---- set membership: x IN (list) and s LIKE pattern ----------------------------------------------------------------------
// Both ask whether a row's value is a member of a set fixed at plan time.  plan_member decides HOW that is carried out.

// LIKE: the whole of `entry` against `pattern`, by code points (utf8_code_points), case-sensitive: % matches zero or more,
// _ exactly one, \ makes the next character literal.  like_pattern_valid is false for a pattern that ends in a lone \.
bool like_pattern_valid(const std::string &pattern);
bool like_match(const std::string &pattern, const std::string &entry);

// Thresholds of a form choice (not API): up to `chain_upto` members are an inline compare chain (QE_IN_CHAIN_UPTO, 0 .. 32; 0 sends
// every list to a table, a measurement switch); integer members whose span max - min is below `bits_span` are a bit table
// (QE_IN_BITS_SPAN, a power of two, at most 2^20: the table is at most 128 KiB).
struct MemberThresholds { int chain_upto; int64_t bits_span; };
MemberThresholds member_thresholds();
constexpr int kMemberChainDefault = 4;   // measured: profiles/member_summary.txt, DESIGN.md 3
constexpr int64_t kMemberBitsSpanDefault = 1ll << 20;
constexpr int kMemberMaxItems = 65536;

// Open-addressing set of 64-bit images, linear probing.  words = {mask | probe << 32, home mask, EMPTY, 0, slots[mask + 1]}:
// the home slot of an image is member_hash(image) & home mask, it is a member iff one of the `probe` slots from its home on
// (wrapping at mask) holds it and it is not EMPTY (a value chosen so that it is no member).  The slots are a power of two
// >= 2 * members; while the longest probe exceeds kMemberProbeBound they are doubled, up to kMemberGrowth times the first size.
// QE_IN_HASH_BITS=<n> (a test switch, read at every build) keeps only the low n bits of the hash in the home mask.
constexpr int kMemberProbeBound = 8;
constexpr int kMemberGrowth = 4;
constexpr int kMemberHashHeader = 4;   // 64-bit words in front of the slots
inline uint32_t member_hash(uint64_t image) { return (uint32_t)((image * 0x9E3779B97F4A7C15ull) >> 32); }
struct MemberHashSet {
    std::vector<uint64_t> words;
    uint64_t mask = 0, home_mask = 0, empty = 0;
    int probe = 0;
    bool contains(uint64_t image) const;   // the probe as the device carries it out
};
MemberHashSet build_member_hash(const std::vector<uint64_t> &images);

// java.lang.Double.doubleToLongBits
uint64_t canonical_bits(double d);

struct MemberPlan {
    // Constant: `value` for every row.  Copy / Negate: a BOOLEAN value itself / its negation.  Chain: value == chain[0] || ...
    // Bits: bit (value - base) of `table` (32-bit words), false outside [0, nbits).  Hash: `table` holds a MemberHashSet's words
    // as pairs of 32-bit words, low word first.  In every case the result is NULL exactly where the value is.
    enum Kind { Constant, Copy, Negate, Chain, Bits, Hash } kind = Constant;
    bool value = false;
    // What chain / base / the hashed images are compared with: the dictionary code of a STRING value; the INTEGER operand of the
    // value's cast (on_int); else the canonical bits of the DOUBLE value.
    bool on_int = false;
    std::vector<int64_t> chain;
    int64_t base = 0, nbits = 0;
    std::vector<int32_t> table;
};
// The IN or LIKE node `id` of `e`.  `value`: the side of a STRING value (its dictionary, or a bare literal), unused otherwise.
// `int_type`: QE_INT64 / QE_INT32 when the value is a cast of an integer expression to DOUBLE, else -1.
MemberPlan plan_member(const Expr &e, int id, const StrSide &value, int int_type);
// Per node id: the IN / LIKE nodes over a bare STRING column (col_dicts[c] = dictionary of batch column c) that plan_member folds
// to a constant.  Such a node reads its column through the validity alone (column_uses' `validity_only`).
std::vector<char> constant_column_members(const Expr &e, const std::vector<std::shared_ptr<DictData>> &col_dicts);
// (for the tests) the numeric decision on its own
MemberPlan plan_numeric_member(const std::vector<double> &literals, int int_type);

}  // namespace qe
