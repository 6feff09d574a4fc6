// member_rules_test.cpp -- the set-membership rules of qe_expr_rules.h (plan_member, the LIKE matcher, the hash set) against
// values written out by hand.  Host only: built with g++ against the checkout's qe_internal.h and libqe_hip.so and run by
// tests/test_member_rules_cpu.py; never touches a device.
#include "qe_expr_rules.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

using namespace qe;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);              \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static std::shared_ptr<DictData> dict_of(const std::vector<std::string> &entries) {
    auto d = std::make_shared<DictData>();
    for (const std::string &s : entries) {
        d->index[s] = (int32_t)d->entries.size();
        d->entries.push_back(s);
    }
    return d;
}
// value node (a column), second operand, function node -- children before parents, as decode_program appends them
static Expr member_expr(int fn, int value_type, Node second) {
    Expr e;
    Node v;
    v.kind = N_COLUMN; v.col = 0; v.type = value_type;
    e.nodes.push_back(v);
    e.nodes.push_back(second);
    Node f;
    f.kind = N_FN; f.fn = fn; f.type = QE_BOOLEAN; f.ops = {0, 1};
    e.nodes.push_back(f);
    e.root = 2;
    return e;
}
static Node str_list(const std::vector<std::string> &items) {
    Node n;
    n.kind = N_LIST; n.type = QE_STRING; n.list_str = items;
    return n;
}
static Node bool_list(const std::vector<char> &items) {
    Node n;
    n.kind = N_LIST; n.type = QE_BOOLEAN; n.list_bool = items;
    return n;
}
static Node pattern(const std::string &p) {
    Node n;
    n.kind = N_STR; n.type = QE_STRING; n.str = p;
    return n;
}
static bool bit(const MemberPlan &p, int64_t v) {
    const uint64_t i = (uint64_t)v - (uint64_t)p.base;
    return i < (uint64_t)p.nbits && ((uint32_t)p.table[(size_t)(i >> 5)] >> (i & 31) & 1u);
}
static MemberHashSet hash_of(const MemberPlan &p) {   // the table words of a Hash plan back as a set
    MemberHashSet h;
    for (size_t i = 0; i + 1 < p.table.size(); i += 2) h.words.push_back((uint64_t)(uint32_t)p.table[i] | ((uint64_t)(uint32_t)p.table[i + 1] << 32));
    h.mask = h.words[0] & 0xffffffffull;
    h.probe = (int)(h.words[0] >> 32);
    h.home_mask = h.words[1];
    h.empty = h.words[2];
    return h;
}

static void test_like_matcher() {
    struct { const char *p, *s; bool want; } t[] = {
        {"", "", true}, {"", "a", false}, {"a", "", false}, {"%", "", true}, {"%", "anything", true}, {"%%", "", true}, {"%%", "xy", true},
        {"_", "", false}, {"_", "a", true}, {"_", "ab", false}, {"_", "\xF0\x9F\x98\x80", true},   // one supplementary character is ONE code point
        {"__", "\xF0\x9F\x98\x80", false}, {"_", "\xC3\xA9", true}, {"caf_", "caf\xC3\xA9", true},
        {"JFK%", "JFK", true}, {"JFK%", "JFK Airport", true}, {"JFK%", "LGA JFK", false}, {"JFK%", "JF", false},
        {"%port", "Airport", true}, {"%port", "ports", false}, {"%or%", "Airport", true}, {"%or%", "or", true}, {"%or%", "o r", false},
        {"a%b%c", "abc", true}, {"a%b%c", "a__b__c", true}, {"a%b%c", "acb", false}, {"a%b", "abab", true}, {"a%a", "a", false},
        {"100\\%", "100%", true}, {"100\\%", "1000", false}, {"a\\_b", "a_b", true}, {"a\\_b", "axb", false}, {"\\\\", "\\", true},
        {"\\a", "a", true}, {"abc", "abc", true}, {"abc", "ABC", false}, {"abc", "abcd", false}, {"%\n%", "a\nb", true},
        {"_", "\xFF", true}, {"__", "\xFF\xFE", true},   // invalid bytes: each its own unit
    };
    for (const auto &c : t) {
        if (like_match(c.p, c.s) != c.want) {
            std::printf("FAIL like_match('%s', '%s') != %d\n", c.p, c.s, (int)c.want);
            failures++;
        }
    }
    CHECK(like_pattern_valid("") && like_pattern_valid("a\\\\") && like_pattern_valid("\\%"));
    CHECK(!like_pattern_valid("\\") && !like_pattern_valid("abc\\") && !like_pattern_valid("a\\\\\\"));
    int code = 0;
    try { like_match("abc\\", "abc"); } catch (const Error &e) { code = e.code; }
    CHECK(code == QE_ERR_PROGRAM);
}

static void test_string_routes() {
    std::vector<std::string> entries;
    for (int i = 0; i < 100; i++) entries.push_back("k" + std::to_string(i));
    const auto d = dict_of(entries);
    const StrSide side{d.get(), nullptr};
    const int K = member_thresholds().chain_upto;
    CHECK(K >= 2 && K <= 32);
    // IN: absent literals drop out; 0 / 1 / <= K / > K / every code
    Expr e = member_expr(QE_FN_IN, QE_STRING, str_list({"absent", "nope"}));
    MemberPlan p = plan_member(e, 2, side, -1);
    CHECK(p.kind == MemberPlan::Constant && !p.value);
    e = member_expr(QE_FN_IN, QE_STRING, str_list({"k7", "absent", "k7"}));
    p = plan_member(e, 2, side, -1);
    CHECK(p.kind == MemberPlan::Chain && p.chain == std::vector<int64_t>{7} && !p.on_int);
    e = member_expr(QE_FN_IN, QE_STRING, str_list({"k9", "k3"}));
    p = plan_member(e, 2, side, -1);
    CHECK(p.kind == MemberPlan::Chain && (p.chain == std::vector<int64_t>{3, 9}));
    std::vector<std::string> many(entries.begin() + 10, entries.begin() + 10 + 40);
    many.push_back("absent");
    e = member_expr(QE_FN_IN, QE_STRING, str_list(many));
    p = plan_member(e, 2, side, -1);
    CHECK(p.kind == MemberPlan::Bits && p.base == 0 && p.nbits == 100 && p.table.size() == 4);
    for (int c = -3; c < 140; c++) CHECK(bit(p, c) == (c >= 10 && c < 50));
    e = member_expr(QE_FN_IN, QE_STRING, str_list(entries));
    p = plan_member(e, 2, side, -1);
    CHECK(p.kind == MemberPlan::Constant && p.value);
    // a literal value folds
    const std::string lit = "k3";
    e = member_expr(QE_FN_IN, QE_STRING, str_list({"k9", "k3"}));
    p = plan_member(e, 2, StrSide{nullptr, &lit}, -1);
    CHECK(p.kind == MemberPlan::Constant && p.value);
    e = member_expr(QE_FN_LIKE, QE_STRING, pattern("k_"));
    p = plan_member(e, 2, StrSide{nullptr, &lit}, -1);
    CHECK(p.kind == MemberPlan::Constant && p.value);
    // LIKE over the dictionary: k1% = k1, k10 .. k19 (11 codes); k% = all; z% = none; no wildcard = that one entry
    e = member_expr(QE_FN_LIKE, QE_STRING, pattern("k1%"));
    p = plan_member(e, 2, side, -1);
    if (K >= 11) {
        CHECK(p.kind == MemberPlan::Chain && p.chain.size() == 11 && p.chain[0] == 1 && p.chain[1] == 10 && p.chain[10] == 19);
    } else {
        CHECK(p.kind == MemberPlan::Bits && p.nbits == 100);
        for (int c = 0; c < 100; c++) CHECK(bit(p, c) == (c == 1 || (c >= 10 && c <= 19)));
    }
    e = member_expr(QE_FN_LIKE, QE_STRING, pattern("k%"));
    p = plan_member(e, 2, side, -1);
    CHECK(p.kind == MemberPlan::Constant && p.value);
    e = member_expr(QE_FN_LIKE, QE_STRING, pattern("z%"));
    p = plan_member(e, 2, side, -1);
    CHECK(p.kind == MemberPlan::Constant && !p.value);
    e = member_expr(QE_FN_LIKE, QE_STRING, pattern("k42"));
    p = plan_member(e, 2, side, -1);
    CHECK(p.kind == MemberPlan::Chain && p.chain == std::vector<int64_t>{42});
    // constant_column_members marks exactly the folded nodes over a bare column
    e = member_expr(QE_FN_LIKE, QE_STRING, pattern("k%"));
    CHECK((constant_column_members(e, {d}) == std::vector<char>{0, 0, 1}));
    e = member_expr(QE_FN_LIKE, QE_STRING, pattern("k1%"));
    CHECK((constant_column_members(e, {d}) == std::vector<char>{0, 0, 0}));
    // BOOLEAN
    e = member_expr(QE_FN_IN, QE_BOOLEAN, bool_list({1, 1}));
    CHECK(plan_member(e, 2, StrSide{nullptr, nullptr}, -1).kind == MemberPlan::Copy);
    e = member_expr(QE_FN_IN, QE_BOOLEAN, bool_list({0}));
    CHECK(plan_member(e, 2, StrSide{nullptr, nullptr}, -1).kind == MemberPlan::Negate);
    e = member_expr(QE_FN_IN, QE_BOOLEAN, bool_list({0, 1}));
    p = plan_member(e, 2, StrSide{nullptr, nullptr}, -1);
    CHECK(p.kind == MemberPlan::Constant && p.value);
}

static void test_numeric_routes() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double two53 = 9007199254740992.0;
    // integer route: NaN, +-Inf, a fraction and -0.0 can never equal a converted integer and drop out
    MemberPlan p = plan_numeric_member({5.0, nan, inf, -inf, 2.5, -0.0, 5.0, -7.0}, QE_INT64);
    CHECK(p.kind == MemberPlan::Chain && p.on_int && (p.chain == std::vector<int64_t>{-7, 5}));
    p = plan_numeric_member({nan, 0.5, -0.0}, QE_INT64);
    CHECK(p.kind == MemberPlan::Constant && !p.value);
    p = plan_numeric_member({0.0, -0.0}, QE_INT32);
    CHECK(p.kind == MemberPlan::Chain && p.on_int && p.chain == std::vector<int64_t>{0});
    // an INT32 value: literals outside its range drop out too, whatever their size
    p = plan_numeric_member({1.0, 2147483648.0, -2147483649.0, two53}, QE_INT32);
    CHECK(p.kind == MemberPlan::Chain && p.on_int && p.chain == std::vector<int64_t>{1});
    // |L| >= 2^53: several integers convert to L, the test runs on the double images of the cast value
    p = plan_numeric_member({two53, 1.0}, QE_INT64);
    CHECK(p.kind == MemberPlan::Chain && !p.on_int && p.chain.size() == 2);
    CHECK((uint64_t)p.chain[0] == canonical_bits(1.0) && (uint64_t)p.chain[1] == canonical_bits(two53));
    p = plan_numeric_member({-two53}, QE_INT64);
    CHECK(!p.on_int);
    p = plan_numeric_member({two53 - 1.0}, QE_INT64);
    CHECK(p.on_int && p.chain == std::vector<int64_t>{9007199254740991ll});
    // DOUBLE values: canonical images, one NaN, two zeros
    p = plan_numeric_member({nan, -nan, 0.0, -0.0}, -1);
    CHECK(p.kind == MemberPlan::Chain && !p.on_int && p.chain.size() == 3);
    CHECK(canonical_bits(nan) == 0x7ff8000000000000ull && canonical_bits(-nan) == 0x7ff8000000000000ull);
    CHECK(canonical_bits(-0.0) == 0x8000000000000000ull && canonical_bits(0.0) == 0);
    // bit table: span below S; the edge
    const int64_t S = member_thresholds().bits_span;
    CHECK(S == (1ll << 20));
    std::vector<double> narrow;
    for (int i = 0; i < 40; i++) narrow.push_back(100.0 + 3 * i);
    p = plan_numeric_member(narrow, QE_INT64);
    CHECK(p.kind == MemberPlan::Bits && p.on_int && p.base == 100 && p.nbits == 118);
    for (int v = 90; v < 230; v++) CHECK(bit(p, v) == (v >= 100 && v <= 217 && (v - 100) % 3 == 0));
    CHECK(!bit(p, std::numeric_limits<int64_t>::min()) && !bit(p, std::numeric_limits<int64_t>::max()));
    for (int64_t span : {S - 2, S - 1, S}) {
        std::vector<double> edge = narrow;
        edge.push_back(100.0 + (double)span);
        p = plan_numeric_member(edge, QE_INT64);
        CHECK(p.kind == (span < S ? MemberPlan::Bits : MemberPlan::Hash));
        if (span < S) CHECK(p.nbits == span + 1 && (int64_t)p.table.size() * 4 <= 128 * 1024 && bit(p, 100 + span) && !bit(p, 101 + span));
    }
    // hash set: every literal found within the probe length, EMPTY no member, no non-member found
    std::vector<double> wide;
    for (int i = 0; i < 40; i++) wide.push_back((double)((int64_t)i * 1000003 - 17000000));
    p = plan_numeric_member(wide, QE_INT64);
    CHECK(p.kind == MemberPlan::Hash && p.on_int);
    MemberHashSet h = hash_of(p);
    CHECK(h.mask + 1 >= 80 && ((h.mask + 1) & h.mask) == 0 && h.words.size() == (size_t)kMemberHashHeader + h.mask + 1);
    CHECK(h.probe >= 1 && h.probe <= kMemberProbeBound && h.home_mask == h.mask);
    for (double v : wide) CHECK(h.contains((uint64_t)(int64_t)v));
    CHECK(!h.contains(h.empty));
    for (int64_t v = -17000100; v < -16999900; v++) CHECK(h.contains((uint64_t)v) == (v == -17000000));
    size_t empties = 0;
    for (size_t i = kMemberHashHeader; i < h.words.size(); i++) empties += h.words[i] == h.empty;
    CHECK(empties == h.mask + 1 - 40);
    // EMPTY moves off a member
    MemberHashSet g = build_member_hash({0xfff7ffffffffffffull, 0xfff7fffffffffffeull, 5});
    CHECK(g.empty == 0xfff7fffffffffffdull && g.contains(0xfff7ffffffffffffull) && g.contains(5) && !g.contains(g.empty));
    // the table depends on the set alone: order and duplicates of the list do not matter
    std::vector<double> shuffled(wide.rbegin(), wide.rend());
    shuffled.push_back(wide[3]);
    CHECK(plan_numeric_member(shuffled, QE_INT64).table == p.table);
    // DOUBLE images
    std::vector<double> dl;
    for (int i = 0; i < 33; i++) dl.push_back(i + 0.5);
    dl.push_back(nan);
    dl.push_back(-0.0);
    p = plan_numeric_member(dl, -1);
    CHECK(p.kind == MemberPlan::Hash && !p.on_int);
    h = hash_of(p);
    CHECK(h.contains(canonical_bits(nan)) && h.contains(canonical_bits(-0.0)) && !h.contains(canonical_bits(0.0)) && h.contains(canonical_bits(7.5)));
    // growth under QE_IN_HASH_BITS=2: four home slots, the probe length is the set's size whatever the slots; the builder doubles
    // kMemberGrowth-fold and then accepts it
    setenv("QE_IN_HASH_BITS", "2", 1);
    std::vector<uint64_t> images;
    for (uint64_t i = 0; i < 48; i++) images.push_back(i * 7919 + 1);
    g = build_member_hash(images);
    CHECK(g.home_mask == 3 && g.mask + 1 == 128 * (uint64_t)kMemberGrowth && g.probe > kMemberProbeBound && g.probe <= 48);
    for (uint64_t im : images) CHECK(g.contains(im));
    for (uint64_t i = 0; i < 48; i++) CHECK(!g.contains(i * 7919 + 2));
    unsetenv("QE_IN_HASH_BITS");
    g = build_member_hash(images);
    CHECK(g.home_mask == g.mask && g.mask + 1 >= 128 && g.probe <= kMemberProbeBound);
    // thresholds from the environment: K clamps to 0 .. 32, S takes powers of two up to 2^20 only
    setenv("QE_IN_CHAIN_UPTO", "0", 1);
    CHECK(member_thresholds().chain_upto == 0 && plan_numeric_member({1.0, 2.0}, QE_INT64).kind == MemberPlan::Bits);
    CHECK(plan_numeric_member({1.5}, -1).kind == MemberPlan::Hash);
    setenv("QE_IN_CHAIN_UPTO", "99", 1);
    CHECK(member_thresholds().chain_upto == 32);
    unsetenv("QE_IN_CHAIN_UPTO");
    setenv("QE_IN_BITS_SPAN", "64", 1);
    CHECK(member_thresholds().bits_span == 64 && plan_numeric_member(narrow, QE_INT64).kind == MemberPlan::Hash);
    setenv("QE_IN_BITS_SPAN", "4194304", 1);
    CHECK(member_thresholds().bits_span == (1ll << 20));
    unsetenv("QE_IN_BITS_SPAN");
}

int main() {
    test_like_matcher();
    test_string_routes();
    test_numeric_routes();
    if (failures) {
        std::printf("%d membership rule checks FAILED\n", failures);
        return 1;
    }
    std::printf("all membership rule checks passed\n");
    return 0;
}
