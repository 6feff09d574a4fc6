// expr_rules_test.cpp -- the plan-time rules of qe_expr_rules.h against values written out by hand.  Host only: built with g++
// against the checkout's qe_internal.h and libqe_hip.so and run by tests/test_expr_rules_cpu.py; never touches a device.
#include "qe_expr_rules.h"

#include <cmath>
#include <cstdio>

using namespace qe;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);              \
            failures++;                                                      \
        }                                                                    \
    } while (0)

// nodes are appended the way decode_program does: children before parents, left to right
static int column(Expr &e, int col, int type) {
    Node n;
    n.kind = N_COLUMN; n.col = col; n.type = type;
    e.nodes.push_back(n);
    return e.root = (int)e.nodes.size() - 1;
}
static int fn(Expr &e, int f, int type, std::vector<int> ops) {
    Node n;
    n.kind = N_FN; n.fn = f; n.type = type; n.ops = std::move(ops);
    e.nodes.push_back(n);
    return e.root = (int)e.nodes.size() - 1;
}
static int number(Expr &e, double v, int type = QE_DOUBLE) {
    Node n;
    n.kind = N_NUM; n.num = v; n.type = type;
    e.nodes.push_back(n);
    return e.root = (int)e.nodes.size() - 1;
}
static int cast(Expr &e, int type, int op) {
    Node n;
    n.kind = N_CAST; n.type = type; n.ops = {op};
    e.nodes.push_back(n);
    return e.root = (int)e.nodes.size() - 1;
}
static std::shared_ptr<DictData> dict_of(const std::vector<std::string> &entries) {
    auto d = std::make_shared<DictData>();
    for (const std::string &s : entries) {
        d->index[s] = (int32_t)d->entries.size();
        d->entries.push_back(s);
    }
    return d;
}
static StrSide dict_side(const std::shared_ptr<DictData> &d) { return StrSide{d.get(), nullptr}; }
static StrSide lit_side(const std::string &s) { return StrSide{nullptr, &s}; }
static bool same_uses(const std::vector<ColumnUse> &got, const std::vector<ColumnUse> &want) {
    if (got.size() != want.size()) return false;
    for (size_t i = 0; i < got.size(); i++)
        if (got[i].col != want[i].col || got[i].value != want[i].value) return false;
    return true;
}
static std::string error_of(const Expr &e, const std::vector<int> &types, int *code) {
    try {
        column_uses(e, e.root, types);
    } catch (const Error &err) {
        *code = err.code;
        return err.msg;
    }
    *code = 0;
    return "no error";
}
static int sign(int x) { return x < 0 ? -1 : x > 0 ? 1 : 0; }

static void test_function_classes() {
    const int fns[6] = {QE_FN_CMP_LT, QE_FN_CMP_LE, QE_FN_CMP_GE, QE_FN_CMP_GT, QE_FN_CMP_EQ, QE_FN_CMP_NE};
    const bool want[6][3] = {{true, false, false}, {true, true, false}, {false, true, true},   // c = -1, 0, 1
                             {false, false, true}, {false, true, false}, {true, false, true}};
    for (int f = 0; f < 6; f++)
        for (int c = -1; c <= 1; c++) CHECK(cmp_holds(fns[f], c) == want[f][c + 1]);
    for (int f = 0; f < QE_FN_COUNT_; f++) {
        CHECK(is_arithmetic_fn(f) == (f == QE_FN_ADD || f == QE_FN_SUB || f == QE_FN_MUL || f == QE_FN_DIV || f == QE_FN_MOD));
        CHECK(is_comparison_fn(f) == (f == fns[0] || f == fns[1] || f == fns[2] || f == fns[3] || f == fns[4] || f == fns[5]));
        CHECK(is_null_test_fn(f) == (f == QE_FN_IS_NULL || f == QE_FN_IS_NOT_NULL));
    }
}

static void test_conjuncts() {
    Expr e;   // (p0 AND (p1 AND (p2 OR p3))) AND p4
    const int p0 = column(e, 0, QE_BOOLEAN), p1 = column(e, 1, QE_BOOLEAN), p2 = column(e, 2, QE_BOOLEAN), p3 = column(e, 3, QE_BOOLEAN);
    const int either = fn(e, QE_FN_OR, QE_BOOLEAN, {p2, p3});
    const int inner = fn(e, QE_FN_AND, QE_BOOLEAN, {p1, either});
    const int left = fn(e, QE_FN_AND, QE_BOOLEAN, {p0, inner});
    const int p4 = column(e, 4, QE_BOOLEAN);
    const int root = fn(e, QE_FN_AND, QE_BOOLEAN, {left, p4});
    CHECK(split_conjuncts(e, root) == (std::vector<int>{p0, p1, either, p4}));
    CHECK(split_conjuncts(e, inner) == (std::vector<int>{p1, either}));
    CHECK(split_conjuncts(e, either) == (std::vector<int>{either}));   // a lone root that is no AND
    CHECK(split_conjuncts(e, p0) == (std::vector<int>{p0}));
}

static void test_column_uses() {
    const std::vector<int> types = {QE_DOUBLE, QE_INT64, QE_STRING, QE_DOUBLE};
    {
        Expr e;   // b IS NULL
        fn(e, QE_FN_IS_NULL, QE_BOOLEAN, {column(e, 1, QE_INT64)});
        CHECK(same_uses(column_uses(e, e.root, types), {{1, false}}));
    }
    {
        Expr e;   // b IS NULL AND b < d   -> b is also read; and s IS NOT NULL, (a + d) IS NULL
        const int t = fn(e, QE_FN_IS_NULL, QE_BOOLEAN, {column(e, 1, QE_INT64)});
        const int b = column(e, 1, QE_INT64), d = column(e, 3, QE_DOUBLE);
        const int lt = fn(e, QE_FN_CMP_LT, QE_BOOLEAN, {b, d});
        const int both = fn(e, QE_FN_AND, QE_BOOLEAN, {t, lt});
        const int sn = fn(e, QE_FN_IS_NOT_NULL, QE_BOOLEAN, {column(e, 2, QE_STRING)});
        const int a = column(e, 0, QE_DOUBLE), d2 = column(e, 3, QE_DOUBLE);
        const int sum = fn(e, QE_FN_ADD, QE_DOUBLE, {a, d2});
        const int en = fn(e, QE_FN_IS_NULL, QE_BOOLEAN, {sum});   // over an expression: its columns are read
        fn(e, QE_FN_AND, QE_BOOLEAN, {fn(e, QE_FN_AND, QE_BOOLEAN, {both, sn}), en});
        CHECK(same_uses(column_uses(e, e.root, types), {{1, false}, {1, true}, {3, true}, {2, false}, {0, true}, {3, true}}));
        CHECK(same_uses(column_uses(e, lt, types), {{1, true}, {3, true}}));     // one subtree
        CHECK(same_uses(column_uses(e, both, types), {{1, false}, {1, true}, {3, true}}));
        CHECK(same_uses(column_uses(e, sn, types), {{2, false}}));
    }
    int code = 0;
    {
        Expr e;
        column(e, 7, QE_DOUBLE);
        CHECK(error_of(e, types, &code) == "column index 7 out of range");
        CHECK(code == QE_ERR_PROGRAM);
    }
    {
        Expr e;
        fn(e, QE_FN_IS_NULL, QE_BOOLEAN, {column(e, 0, QE_INT64)});   // checked under a null test too
        CHECK(error_of(e, types, &code) == "column 0 is DOUBLE in the batch but INT64 in the expression");
        CHECK(code == QE_ERR_PROGRAM);
    }
}

static const std::vector<std::string> kD1 = {"pear", "apple", "fig"}, kD2 = {"kiwi", "apple", "\xF0\x9F\x8D\x8E", ""};   // U+1F34E

static void test_string_compare() {
    const auto d1 = dict_of(kD1), d2 = dict_of(kD2);
    const int fns[6] = {QE_FN_CMP_LT, QE_FN_CMP_LE, QE_FN_CMP_GE, QE_FN_CMP_GT, QE_FN_CMP_EQ, QE_FN_CMP_NE};
    const std::string a = "a", b = "b";
    const bool a_b[6] = {true, true, false, false, false, true}, b_b[6] = {false, true, true, false, true, false},
               b_a[6] = {false, false, true, true, false, true};
    for (int f = 0; f < 6; f++) {
        const StringCompare ab = plan_string_compare(fns[f], lit_side(a), lit_side(b)), bb = plan_string_compare(fns[f], lit_side(b), lit_side(b)),
                            ba = plan_string_compare(fns[f], lit_side(b), lit_side(a));
        CHECK(ab.kind == StringCompare::Constant && ab.value == a_b[f]);
        CHECK(bb.kind == StringCompare::Constant && bb.value == b_b[f]);
        CHECK(ba.kind == StringCompare::Constant && ba.value == b_a[f]);
    }
    const std::string fig = "fig", zz = "zz";
    for (int f : {QE_FN_CMP_EQ, QE_FN_CMP_NE}) {
        StringCompare p = plan_string_compare(f, dict_side(d1), lit_side(fig));   // present: its code
        CHECK(p.kind == StringCompare::Codes && p.lit[1] == 2 && p.table[0].empty() && p.table[1].empty());
        p = plan_string_compare(f, lit_side(zz), dict_side(d2));                  // absent, literal first: -1
        CHECK(p.kind == StringCompare::Codes && p.lit[0] == -1 && p.table[0].empty() && p.table[1].empty());
        p = plan_string_compare(f, lit_side(fig), dict_side(d1));
        CHECK(p.kind == StringCompare::Codes && p.lit[0] == 2);
        p = plan_string_compare(f, dict_side(d1), dict_side(d1));                 // one dictionary: no table
        CHECK(p.kind == StringCompare::Codes && p.table[0].empty() && p.table[1].empty());
    }
    // across the two dictionaries, = included: "" < apple < fig < kiwi < pear < U+1F34E (a surrogate pair, 0xD83C ..)
    for (int f = 0; f < 6; f++) {
        const StringCompare p = plan_string_compare(fns[f], dict_side(d1), dict_side(d2));
        CHECK(p.kind == StringCompare::Ranks);
        CHECK(p.table[0] == (std::vector<int32_t>{4, 1, 2}));
        CHECK(p.table[1] == (std::vector<int32_t>{3, 1, 5, 0}));   // "apple": the same rank on both sides
        for (size_t i = 0; i < kD1.size() && p.table[0].size() == 3 && p.table[1].size() == 4; i++)
            for (size_t j = 0; j < kD2.size(); j++) CHECK(sign(p.table[0][i] - p.table[1][j]) == utf16_compare(kD1[i], kD2[j]));
    }
    {   // an ordering inside ONE dictionary goes through ranks too (codes are not ordered)
        const StringCompare p = plan_string_compare(QE_FN_CMP_LE, dict_side(d1), dict_side(d1));
        CHECK(p.kind == StringCompare::Ranks && p.table[0] == (std::vector<int32_t>{2, 0, 1}) && p.table[1] == p.table[0]);
    }
    {   // an ordering against a literal: apple < b < fig < pear
        StringCompare p = plan_string_compare(QE_FN_CMP_GE, dict_side(d1), lit_side(b));
        CHECK(p.kind == StringCompare::Ranks && p.table[0] == (std::vector<int32_t>{3, 0, 2}) && p.lit[1] == 1 && p.table[1].empty());
        p = plan_string_compare(QE_FN_CMP_LT, lit_side(b), dict_side(d1));
        CHECK(p.kind == StringCompare::Ranks && p.table[1] == (std::vector<int32_t>{3, 0, 2}) && p.lit[0] == 1 && p.table[0].empty());
    }
    {   // compareTo is on UTF-16 code units: the supplementary U+1F34E (0xD83C 0xDF4E) sorts BEFORE U+E000 and U+FFFF, although its
        // UTF-8 bytes (F0 ..) sort after theirs (EE .. / EF ..)
        const std::string e000 = "\xEE\x80\x80", ffff = "\xEF\xBF\xBF";
        CHECK(utf16_compare(kD2[2], e000) < 0 && utf16_compare(kD2[2], ffff) < 0 && kD2[2] > ffff);
        StringCompare p = plan_string_compare(QE_FN_CMP_LT, dict_side(d2), lit_side(e000));   // "" < apple < kiwi < U+1F34E < U+E000
        CHECK(p.kind == StringCompare::Ranks && p.table[0] == (std::vector<int32_t>{2, 1, 3, 0}) && p.lit[1] == 4);
        const auto d3 = dict_of({ffff, "z", e000});
        p = plan_string_compare(QE_FN_CMP_GT, dict_side(d2), dict_side(d3));   // "" apple kiwi z U+1F34E U+E000 U+FFFF
        CHECK(p.table[0] == (std::vector<int32_t>{2, 1, 4, 0}) && p.table[1] == (std::vector<int32_t>{6, 3, 5}));
    }
}

// every entry of `from` has, through `remap` (or unchanged when there is none), the same string in the union
static bool maps_into(const std::vector<std::string> &from, const std::vector<int32_t> *remap, const DictData &u) {
    for (size_t i = 0; i < from.size(); i++) {
        const int32_t c = remap ? (*remap)[i] : (int32_t)i;
        if (c < 0 || (size_t)c >= u.entries.size() || u.entries[(size_t)c] != from[i]) return false;
    }
    return !remap || remap->size() == from.size();
}
static bool index_matches(const DictData &d) {
    for (size_t i = 0; i < d.entries.size(); i++)
        if (d.find(d.entries[i]) != (int32_t)i) return false;
    return d.index.size() == d.entries.size();
}

static void test_dictionary_union() {
    const auto d1 = dict_of(kD1), d2 = dict_of(kD2);
    const std::string fig = "fig", none = "none", x = "x", y = "y";
    {   // column / column over one dictionary
        const DictUnion u = unify_dictionaries(dict_side(d1), dict_side(d1));
        CHECK(!u.remap_second && u.remap.empty() && u.dict->entries == kD1 && index_matches(*u.dict));
        CHECK(u.dict->id != d1->id);
    }
    {   // .. over two: the first one's codes stay, the second one's are remapped
        const DictUnion u = unify_dictionaries(dict_side(d1), dict_side(d2));
        CHECK(u.dict->entries == (std::vector<std::string>{"pear", "apple", "fig", "kiwi", "\xF0\x9F\x8D\x8E", ""}) && index_matches(*u.dict));
        CHECK(u.remap_second && u.remap == (std::vector<int32_t>{3, 1, 4, 5}));
        CHECK(maps_into(kD1, nullptr, *u.dict) && maps_into(kD2, &u.remap, *u.dict));
        CHECK(u.dict->id != d1->id && u.dict->id != d2->id);
        CHECK(d1->entries == kD1 && d2->entries == kD2);   // the inputs are left alone
        const DictUnion v = unify_dictionaries(dict_side(d2), dict_side(d1));   // the other way round
        CHECK(v.dict->entries == (std::vector<std::string>{"kiwi", "apple", "\xF0\x9F\x8D\x8E", "", "pear", "fig"}) && index_matches(*v.dict));
        CHECK(v.remap_second && v.remap == (std::vector<int32_t>{4, 1, 5}) && maps_into(kD2, nullptr, *v.dict) && maps_into(kD1, &v.remap, *v.dict));
        CHECK(v.dict->id != u.dict->id);
    }
    {   // column / literal, present and absent
        DictUnion u = unify_dictionaries(dict_side(d1), lit_side(fig));
        CHECK(!u.remap_second && u.dict->entries == kD1 && u.lit[1] == 2 && u.dict->id != d1->id);
        u = unify_dictionaries(dict_side(d1), lit_side(none));
        CHECK(!u.remap_second && u.dict->entries == (std::vector<std::string>{"pear", "apple", "fig", "none"}) && u.lit[1] == 3);
        CHECK(maps_into(kD1, nullptr, *u.dict) && index_matches(*u.dict) && u.dict->id != d1->id && d1->entries == kD1);
    }
    {   // literal / column: the column's codes stay
        DictUnion u = unify_dictionaries(lit_side(x), dict_side(d2));
        CHECK(!u.remap_second && u.dict->entries == (std::vector<std::string>{"kiwi", "apple", "\xF0\x9F\x8D\x8E", "", "x"}) && u.lit[0] == 4);
        CHECK(maps_into(kD2, nullptr, *u.dict) && index_matches(*u.dict) && u.dict->id != d2->id);
        const std::string empty;
        u = unify_dictionaries(lit_side(empty), dict_side(d2));
        CHECK(!u.remap_second && u.dict->entries == kD2 && u.lit[0] == 3);
    }
    {   // literal / literal
        DictUnion u = unify_dictionaries(lit_side(x), lit_side(y));
        CHECK(!u.remap_second && u.dict->entries == (std::vector<std::string>{"x", "y"}) && u.lit[0] == 0 && u.lit[1] == 1 && index_matches(*u.dict));
        const DictUnion v = unify_dictionaries(lit_side(x), lit_side(x));
        CHECK(v.dict->entries == (std::vector<std::string>{"x"}) && v.lit[0] == 0 && v.lit[1] == 0 && v.dict->id != u.dict->id);
    }
    const auto l = literal_dictionary("lit");
    CHECK(l->entries == (std::vector<std::string>{"lit"}) && l->find("lit") == 0 && index_matches(*l));
}

static void test_exact_integer_literal() {
    const double two53 = 9007199254740992.0;
    long long v = 99;
    CHECK(exact_integer_literal(two53 - 1, v) && v == 9007199254740991ll);
    CHECK(exact_integer_literal(-(two53 - 1), v) && v == -9007199254740991ll);
    CHECK(!exact_integer_literal(two53, v) && !exact_integer_literal(-two53, v));   // strict: 2^53 + 1 converts to 2^53 too
    CHECK(!exact_integer_literal(0.5, v) && !exact_integer_literal(-2.5, v));
    CHECK(!exact_integer_literal(std::nan(""), v) && !exact_integer_literal(INFINITY, v) && !exact_integer_literal(-INFINITY, v));
    CHECK(exact_integer_literal(-0.0, v) && v == 0);
    CHECK(exact_integer_literal(7.0, v) && v == 7);
    CHECK(exact_integer_literal(-2147483649.0, v) && v == -2147483649ll);
    // .. at the width of the integer operand: the INT32 bounds
    CHECK(exact_integer_literal(2147483647.0, QE_INT32, v) && v == 2147483647ll);
    CHECK(exact_integer_literal(-2147483648.0, QE_INT32, v) && v == -2147483648ll);
    CHECK(!exact_integer_literal(2147483648.0, QE_INT32, v) && !exact_integer_literal(-2147483649.0, QE_INT32, v));
    CHECK(exact_integer_literal(2147483648.0, QE_INT64, v) && v == 2147483648ll);
    CHECK(exact_integer_literal(-2147483649.0, QE_INT64, v) && v == -2147483649ll);
    CHECK(exact_integer_literal(two53 - 1, QE_INT64, v) && v == 9007199254740991ll && !exact_integer_literal(two53 - 1, QE_INT32, v));
    CHECK(!exact_integer_literal(two53, QE_INT64, v) && !exact_integer_literal(-two53, QE_INT64, v));   // +-2^53: strict at every width
    CHECK(!exact_integer_literal(two53, QE_INT32, v) && !exact_integer_literal(-two53, QE_INT32, v));
    CHECK(!exact_integer_literal(0.5, QE_INT64, v) && !exact_integer_literal(0.5, QE_INT32, v));
    CHECK(exact_integer_literal(-0.0, QE_INT32, v) && v == 0);
    CHECK(!exact_integer_literal(7.0, QE_DOUBLE, v) && !exact_integer_literal(7.0, -1, v));   // no integer operand: no width
}

static void test_integer_cast_operand() {
    Expr e;
    const int l = column(e, 0, QE_INT64), i = column(e, 1, QE_INT32), d = column(e, 2, QE_DOUBLE), p = column(e, 3, QE_BOOLEAN);
    const int dl = cast(e, QE_DOUBLE, l), di = cast(e, QE_DOUBLE, i);
    CHECK(integer_cast_operand(e, dl) == l && integer_cast_operand(e, di) == i);
    CHECK(integer_cast_operand(e, l) == -1 && integer_cast_operand(e, i) == -1 && integer_cast_operand(e, d) == -1);   // no cast
    const int sum = fn(e, QE_FN_ADD, QE_INT64, {l, cast(e, QE_INT64, i)});
    CHECK(integer_cast_operand(e, sum) == -1);
    CHECK(integer_cast_operand(e, cast(e, QE_DOUBLE, sum)) == sum);                      // any integer expression, not only a column
    const int li = cast(e, QE_INT64, i);
    CHECK(integer_cast_operand(e, li) == -1);                                            // a cast, but not to DOUBLE
    const int dli = cast(e, QE_DOUBLE, li);
    CHECK(integer_cast_operand(e, dli) == li);                                           // a cast of a cast: the inner cast, not the column
    CHECK(integer_cast_operand(e, cast(e, QE_DOUBLE, dl)) == -1);                        // (double)(double)l: the operand is a DOUBLE
    CHECK(integer_cast_operand(e, cast(e, QE_DOUBLE, d)) == -1 && integer_cast_operand(e, cast(e, QE_DOUBLE, p)) == -1);
    const int seven = number(e, 7.0);
    CHECK(integer_cast_operand(e, seven) == -1 && integer_cast_operand(e, cast(e, QE_DOUBLE, seven)) == -1);   // a literal child
    CHECK(integer_cast_operand(e, cast(e, QE_DOUBLE, number(e, 7.0, QE_INT64))) == -1);  // .. whatever type it claims
    CHECK(integer_cast_operand(e, cast(e, QE_DOUBLE, number(e, 7.0, QE_INT32))) == -1);
}

int main() {
    test_function_classes();
    test_conjuncts();
    test_column_uses();
    test_string_compare();
    test_dictionary_union();
    test_exact_integer_literal();
    test_integer_cast_operand();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all expression rule checks passed\n");
    return 0;
}
