// qe_expr_rules.cpp -- the plan-time rules of expression evaluation (see qe_expr_rules.h).
#include "qe_expr_rules.h"

#include <cmath>

namespace qe {

// FilterOperator keeps a row iff the predicate is a non-null TRUE (FilterOperator.kt:20) and a Kleene AND is TRUE iff every
// operand is: the keep mask of the chain is the AND of the conjuncts' keep masks.
std::vector<int> split_conjuncts(const Expr &e, int root) {
    const Node &n = e.nodes[(size_t)root];
    if (!(n.kind == N_FN && n.fn == QE_FN_AND && n.ops.size() == 2)) return {root};
    std::vector<int> left = split_conjuncts(e, n.ops[0]), right = split_conjuncts(e, n.ops[1]);
    left.insert(left.end(), right.begin(), right.end());
    return left;
}

std::vector<ColumnUse> column_uses(const Expr &e, int root, const std::vector<int> &col_types) {
    // children come before their parents: one pass down from the root marks its subtree, one pass up reports the columns in node order
    std::vector<char> inside(e.nodes.size(), 0), null_tested(e.nodes.size(), 0);
    inside[(size_t)root] = 1;
    for (size_t id = (size_t)root + 1; id-- > 0;)
        for (int o : e.nodes[id].ops) {
            inside[(size_t)o] = inside[id];   // (a node has one parent)
            null_tested[(size_t)o] = e.nodes[id].kind == N_FN && is_null_test_fn(e.nodes[id].fn);
        }
    std::vector<ColumnUse> out;
    for (size_t id = 0; id <= (size_t)root; id++) {
        const Node &n = e.nodes[id];
        if (!inside[id] || n.kind != N_COLUMN) continue;
        if (n.col < 0 || n.col >= (int)col_types.size()) fail(QE_ERR_PROGRAM, "column index " + std::to_string(n.col) + " out of range");
        if (col_types[(size_t)n.col] != n.type)
            fail(QE_ERR_PROGRAM, std::string("column ") + std::to_string(n.col) + " is " + type_name(col_types[(size_t)n.col]) +
                                     " in the batch but " + type_name(n.type) + " in the expression");
        out.push_back(ColumnUse{n.col, !null_tested[id]});
    }
    return out;
}

StringCompare plan_string_compare(int fn, const StrSide &a, const StrSide &b) {
    StringCompare p;
    const bool eqne = fn == QE_FN_CMP_EQ || fn == QE_FN_CMP_NE;
    if (a.lit && b.lit) {
        p.value = cmp_holds(fn, utf16_compare(*a.lit, *b.lit));
    } else if (eqne && (a.lit || b.lit)) {
        // String.equals against a literal == code equality; literal absent from the dictionary => never equal (code -1)
        p.kind = StringCompare::Codes;
        if (a.lit) p.lit[0] = b.dict->find(*a.lit);
        else p.lit[1] = a.dict->find(*b.lit);
    } else if (eqne && a.dict == b.dict) {
        p.kind = StringCompare::Codes;
    } else {
        // String.compareTo (BytecodeCompiler.kt:303) / equals across dictionaries: both sides are mapped to their dense rank
        // in ONE merged compareTo order, then the ranks are compared as integers
        p.kind = StringCompare::Ranks;
        const std::vector<std::string> lit_a{a.lit ? *a.lit : ""}, lit_b{b.lit ? *b.lit : ""};
        std::vector<std::vector<int32_t>> ranks = merged_ranks({a.lit ? &lit_a : &a.dict->entries, b.lit ? &lit_b : &b.dict->entries});
        if (a.lit) p.lit[0] = ranks[0][0];
        else p.table[0] = std::move(ranks[0]);
        if (b.lit) p.lit[1] = ranks[1][0];
        else p.table[1] = std::move(ranks[1]);
    }
    return p;
}

static int32_t intern(DictData &d, const std::string &s) {   // the code of `s` in `d`, appended when absent
    const auto at = d.index.emplace(s, (int32_t)d.entries.size());
    if (at.second) d.entries.push_back(s);
    return at.first->second;
}

// The codes of a non-literal first side stay valid (its dictionary is a prefix of the union), the second side's codes are
// remapped when its dictionary is another one, a literal absent from the union is appended.
DictUnion unify_dictionaries(const StrSide &first, const StrSide &second) {
    DictUnion u;
    u.dict = std::make_shared<DictData>();
    const StrSide *base = first.dict ? &first : (second.dict ? &second : nullptr);
    if (base) { *u.dict = *base->dict; u.dict->id = DictData::next_id(); }   // a new dictionary: its own serial number
    u.remap_second = first.dict && second.dict && first.dict != second.dict;
    if (u.remap_second)
        for (const std::string &str : second.dict->entries) u.remap.push_back(intern(*u.dict, str));
    if (first.lit) u.lit[0] = intern(*u.dict, *first.lit);
    if (second.lit) u.lit[1] = intern(*u.dict, *second.lit);
    return u;
}

std::shared_ptr<DictData> literal_dictionary(const std::string &lit) {
    auto d = std::make_shared<DictData>();
    intern(*d, lit);
    return d;
}

bool exact_integer_literal(double lit, long long &out) {
    // STRICT bound: at L = +-2^53 the integers 2^53 and 2^53+1 both convert to L, so (double)(2^53+1) == L although
    // 2^53+1 != L.  Below it every integer x with |x| <= 2^53 converts exactly and every other one converts to a double
    // beyond +-2^53, i.e. on the same side of L as x itself: the conversion is monotone and L is exact.
    if (lit != std::floor(lit) || !(std::fabs(lit) < 9007199254740992.0)) return false;
    out = (long long)lit;
    return true;
}

}  // namespace qe
