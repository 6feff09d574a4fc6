// qe_expr_rules.cpp -- the plan-time rules of expression evaluation (see qe_expr_rules.h).
#include "qe_expr_rules.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

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

std::vector<ColumnUse> column_uses(const Expr &e, int root, const std::vector<int> &col_types, const std::vector<char> *validity_only) {
    // children come before their parents: one pass down from the root marks its subtree, one pass up reports the columns in node order
    std::vector<char> inside(e.nodes.size(), 0), null_tested(e.nodes.size(), 0);
    inside[(size_t)root] = 1;
    for (size_t id = (size_t)root + 1; id-- > 0;)
        for (int o : e.nodes[id].ops) {
            inside[(size_t)o] = inside[id];   // (a node has one parent)
            null_tested[(size_t)o] = e.nodes[id].kind == N_FN && (is_null_test_fn(e.nodes[id].fn) || (validity_only && (*validity_only)[id]));
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

bool exact_integer_literal(double lit, int int_type, long long &out) {
    return exact_integer_literal(lit, out) && (int_type == QE_INT64 || (int_type == QE_INT32 && out >= INT32_MIN && out <= INT32_MAX));
}

int integer_cast_operand(const Expr &e, int id) {
    const Node &x = e.nodes[(size_t)id];
    if (x.kind != N_CAST || x.type != QE_DOUBLE) return -1;
    const Node &c = e.nodes[(size_t)x.ops[0]];
    return (c.type == QE_INT64 || c.type == QE_INT32) && c.kind != N_NUM ? x.ops[0] : -1;
}

// ---- set membership ------------------------------------------------------------------------------------------------------
namespace {
struct LikeItem { enum Kind { Lit, One, Any } kind; uint32_t cp; };
// false: the pattern ends in a lone backslash
bool like_items(const std::string &pattern, std::vector<LikeItem> &items) {
    const std::vector<uint32_t> p = utf8_code_points(pattern);
    for (size_t i = 0; i < p.size(); i++) {
        if (p[i] == '\\') {
            if (++i == p.size()) return false;
            items.push_back(LikeItem{LikeItem::Lit, p[i]});
        } else if (p[i] == '%') {
            if (items.empty() || items.back().kind != LikeItem::Any) items.push_back(LikeItem{LikeItem::Any, 0});   // %% is %
        } else if (p[i] == '_') {
            items.push_back(LikeItem{LikeItem::One, 0});
        } else {
            items.push_back(LikeItem{LikeItem::Lit, p[i]});
        }
    }
    return true;
}
bool like_match_items(const std::vector<LikeItem> &it, const std::vector<uint32_t> &s) {
    // greedy with one point of return: the last % seen and the position it was tried at
    size_t i = 0, j = 0, star = (size_t)-1, mark = 0;
    while (j < s.size()) {
        if (i < it.size() && (it[i].kind == LikeItem::One || (it[i].kind == LikeItem::Lit && it[i].cp == s[j]))) {
            i++;
            j++;
        } else if (i < it.size() && it[i].kind == LikeItem::Any) {
            star = i++;
            mark = j;
        } else if (star != (size_t)-1) {
            i = star + 1;
            j = ++mark;
        } else {
            return false;
        }
    }
    while (i < it.size() && it[i].kind == LikeItem::Any) i++;
    return i == it.size();
}
}  // namespace

bool like_pattern_valid(const std::string &pattern) {
    std::vector<LikeItem> items;
    return like_items(pattern, items);
}

bool like_match(const std::string &pattern, const std::string &entry) {
    std::vector<LikeItem> items;
    if (!like_items(pattern, items)) fail(QE_ERR_PROGRAM, "LIKE pattern ends in a lone \\");
    return like_match_items(items, utf8_code_points(entry));
}

MemberThresholds member_thresholds() {
    MemberThresholds t{kMemberChainDefault, kMemberBitsSpanDefault};
    if (const char *k = std::getenv("QE_IN_CHAIN_UPTO")) t.chain_upto = std::min(32, std::max(0, std::atoi(k)));
    if (const char *sp = std::getenv("QE_IN_BITS_SPAN")) {
        const long long v = std::atoll(sp);
        if (v >= 1 && v <= kMemberBitsSpanDefault && (v & (v - 1)) == 0) t.bits_span = v;
    }
    return t;
}

uint64_t canonical_bits(double d) {
    if (d != d) return 0x7ff8000000000000ull;
    uint64_t b;
    std::memcpy(&b, &d, 8);
    return b;
}

bool MemberHashSet::contains(uint64_t image) const {
    bool found = false;
    const uint64_t home = member_hash(image) & home_mask;
    for (int j = 0; j < probe; j++) found = found || words[(size_t)kMemberHashHeader + ((home + (uint64_t)j) & mask)] == image;
    return found && image != empty;
}

MemberHashSet build_member_hash(const std::vector<uint64_t> &images_in) {
    std::vector<uint64_t> images = images_in;   // sorted and distinct: the table depends on the set alone
    std::sort(images.begin(), images.end());
    images.erase(std::unique(images.begin(), images.end()), images.end());
    MemberHashSet h;
    h.empty = 0xfff7ffffffffffffull;   // (no canonical image of a DOUBLE; any integer may be it)
    while (std::binary_search(images.begin(), images.end(), h.empty)) h.empty--;
    uint64_t hash_bits = ~0ull;
    if (const char *hb = std::getenv("QE_IN_HASH_BITS")) {
        const int n = std::atoi(hb);
        if (n >= 0 && n < 32) hash_bits = (1ull << n) - 1;
    }
    uint64_t slots = 2;
    while (slots < 2 * (uint64_t)images.size()) slots *= 2;
    const uint64_t limit = slots * (uint64_t)kMemberGrowth;
    for (;; slots *= 2) {
        h.mask = slots - 1;
        h.home_mask = h.mask & hash_bits;
        h.probe = 1;
        h.words.assign((size_t)kMemberHashHeader + (size_t)slots, h.empty);
        std::vector<char> used((size_t)slots, 0);
        for (uint64_t image : images) {
            uint64_t at = member_hash(image) & h.home_mask;
            int d = 1;
            for (; used[(size_t)at]; at = (at + 1) & h.mask) d++;
            used[(size_t)at] = 1;
            h.words[(size_t)kMemberHashHeader + (size_t)at] = image;
            h.probe = std::max(h.probe, d);
        }
        if (h.probe <= kMemberProbeBound || slots * 2 > limit) break;   // past the limit the probe length is what it is
    }
    h.words[0] = h.mask | ((uint64_t)h.probe << 32);
    h.words[1] = h.home_mask;
    h.words[2] = h.empty;
    h.words[3] = 0;
    return h;
}

namespace {
std::vector<int32_t> word_pairs(const std::vector<uint64_t> &w) {
    std::vector<int32_t> out;
    out.reserve(w.size() * 2);
    for (uint64_t x : w) {
        out.push_back((int32_t)(uint32_t)x);
        out.push_back((int32_t)(uint32_t)(x >> 32));
    }
    return out;
}

// members = sorted distinct values (dictionary codes or integers) of which `domain` exist in all (0: unknown)
MemberPlan plan_value_set(const std::vector<int64_t> &members, int64_t domain, bool codes) {
    const MemberThresholds th = member_thresholds();
    MemberPlan p;
    p.on_int = !codes;
    const int64_t m = (int64_t)members.size();
    if (m == 0) return p;   // constant false
    if (codes && m == domain) {
        p.value = true;
        return p;
    }
    if ((codes && m == 1) || m <= th.chain_upto) {
        p.kind = MemberPlan::Chain;
        p.chain = members;
        return p;
    }
    const uint64_t span = (uint64_t)members.back() - (uint64_t)members.front();
    if (codes || span < (uint64_t)th.bits_span) {
        p.kind = MemberPlan::Bits;
        p.base = codes ? 0 : members.front();
        p.nbits = codes ? domain : (int64_t)span + 1;
        p.table.assign((size_t)((p.nbits + 31) / 32), 0);
        for (int64_t v : members) {
            const uint64_t i = (uint64_t)v - (uint64_t)p.base;
            p.table[(size_t)(i >> 5)] |= (int32_t)(1u << (i & 31));
        }
        return p;
    }
    p.kind = MemberPlan::Hash;
    std::vector<uint64_t> images(members.begin(), members.end());
    p.table = word_pairs(build_member_hash(images).words);
    return p;
}

MemberPlan plan_code_member(const std::vector<char> &member) {
    std::vector<int64_t> codes;
    for (size_t c = 0; c < member.size(); c++)
        if (member[c]) codes.push_back((int64_t)c);
    return plan_value_set(codes, (int64_t)member.size(), true);
}
}  // namespace

MemberPlan plan_numeric_member(const std::vector<double> &literals, int int_type) {
    if (int_type == QE_INT64 || int_type == QE_INT32) {
        // (double)x == L on the integers: a literal no converted integer equals is dropped -- NaN, +-Inf, a fraction, -0.0 (every
        // converted integer is +0.0 or nonzero), a value outside an INT32 value's range.  At |L| >= 2^53 several integers convert
        // to L: one such literal sends the whole test to the double images of the cast value.
        std::vector<int64_t> ints;
        bool exact = true;
        for (double lit : literals) {
            long long v = 0;
            if (lit != lit || std::isinf(lit) || lit != std::floor(lit) || (lit == 0.0 && std::signbit(lit))) continue;
            if (int_type == QE_INT32 && (lit < -2147483648.0 || lit > 2147483647.0)) continue;
            if (!exact_integer_literal(lit, v)) { exact = false; break; }
            ints.push_back(v);
        }
        if (exact) {
            std::sort(ints.begin(), ints.end());
            ints.erase(std::unique(ints.begin(), ints.end()), ints.end());
            return plan_value_set(ints, 0, false);
        }
    }
    std::vector<uint64_t> images;
    for (double lit : literals) images.push_back(canonical_bits(lit));
    std::sort(images.begin(), images.end());
    images.erase(std::unique(images.begin(), images.end()), images.end());
    MemberPlan p;
    if ((int)images.size() <= member_thresholds().chain_upto) {
        p.kind = MemberPlan::Chain;
        for (uint64_t i : images) p.chain.push_back((int64_t)i);
    } else {
        p.kind = MemberPlan::Hash;
        p.table = word_pairs(build_member_hash(images).words);
    }
    return p;
}

std::vector<char> constant_column_members(const Expr &e, const std::vector<std::shared_ptr<DictData>> &col_dicts) {
    std::vector<char> out(e.nodes.size(), 0);
    for (size_t id = 0; id < e.nodes.size(); id++) {
        const Node &n = e.nodes[id];
        if (n.kind != N_FN || (n.fn != QE_FN_IN && n.fn != QE_FN_LIKE)) continue;
        const Node &v = e.nodes[(size_t)n.ops[0]];
        if (v.kind != N_COLUMN || v.type != QE_STRING || v.col < 0 || v.col >= (int)col_dicts.size() || !col_dicts[(size_t)v.col]) continue;
        out[id] = plan_member(e, (int)id, StrSide{col_dicts[(size_t)v.col].get(), nullptr}, -1).kind == MemberPlan::Constant;
    }
    return out;
}

MemberPlan plan_member(const Expr &e, int id, const StrSide &value, int int_type) {
    const Node &n = e.nodes[(size_t)id];
    const Node &second = e.nodes[(size_t)n.ops[1]];
    MemberPlan p;
    if (n.fn == QE_FN_LIKE) {
        const std::string &pattern = second.str;
        if (value.lit) {
            p.value = like_match(pattern, *value.lit);
            return p;
        }
        std::vector<char> member(value.dict->entries.size(), 0);
        for (size_t c = 0; c < member.size(); c++) member[c] = like_match(pattern, value.dict->entries[c]);
        return plan_code_member(member);
    }
    if (second.type == QE_STRING) {
        if (value.lit) {
            p.value = std::find(second.list_str.begin(), second.list_str.end(), *value.lit) != second.list_str.end();
            return p;
        }
        std::vector<char> member(value.dict->entries.size(), 0);
        for (const std::string &lit : second.list_str) {   // String.equals against a literal == code equality; an absent literal drops out
            const int32_t c = value.dict->find(lit);
            if (c >= 0) member[(size_t)c] = 1;
        }
        return plan_code_member(member);
    }
    if (second.type == QE_BOOLEAN) {
        bool t = false, f = false;
        for (char b : second.list_bool) (b ? t : f) = true;
        if (t && f) p.value = true;
        else p.kind = t ? MemberPlan::Copy : MemberPlan::Negate;
        return p;
    }
    return plan_numeric_member(second.list_num, int_type);
}

}  // namespace qe
