// group_finish_test.cpp -- the group entry rules of qe_group_finish.h against values written out by hand: every expectation is
// exact.  Host only: built with g++ against the checkout's header and libqe_hip.so and run by tests/test_group_finish_cpu.py;
// never touches a device.
#include "qe_group_finish.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <utility>

using namespace qe;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAIL line %d: %s\n", __LINE__, #cond);              \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static uint64_t bits_of(double d) { uint64_t b; std::memcpy(&b, &d, 8); return b; }
static double double_of(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }
// the ordered key as the kernels build it
static uint64_t ordered_key(double d) {
    const int64_t b = (int64_t)bits_of(d);
    return (uint64_t)(b ^ ((b >> 63) & 0x7fffffffffffffffll));
}
static const double kInf = std::numeric_limits<double>::infinity();
static const uint64_t kNaNBits = 0x7ff8000000000123ull;

static void test_identity_and_finish() {
    CHECK(agg_identity(QE_AGG_MIN) == 0x7fffffffffffffffull);
    CHECK(agg_identity(QE_AGG_MAX) == 0x8000000000000000ull);
    CHECK(agg_identity(QE_AGG_SUM) == 0 && agg_identity(QE_AGG_AVG) == 0 && agg_identity(QE_AGG_COUNT) == 0);
    // the identities are the ends of key space: every key, the infinities' included, lies strictly inside
    CHECK((int64_t)ordered_key(kInf) < (int64_t)agg_identity(QE_AGG_MIN) && (int64_t)ordered_key(-kInf) > (int64_t)agg_identity(QE_AGG_MAX));

    double v = -1.0;
    CHECK(finish_accumulator(QE_AGG_COUNT, 0, 0, v) && bits_of(v) == bits_of(0.0));       // COUNT is valid at count 0
    CHECK(finish_accumulator(QE_AGG_COUNT, 7, 12345, v) && v == 7.0);
    const int nullable[] = {QE_AGG_SUM, QE_AGG_AVG, QE_AGG_MIN, QE_AGG_MAX};
    for (int fn : nullable) {                                                             // NULL with value 0.0 at count 0
        v = -1.0;
        CHECK(!finish_accumulator(fn, 0, agg_identity(fn), v) && bits_of(v) == bits_of(0.0));
        v = -1.0;
        CHECK(!finish_accumulator(fn, 0, bits_of(3.5), v) && bits_of(v) == bits_of(0.0));
    }
    CHECK(finish_accumulator(QE_AGG_SUM, 4, bits_of(10.0), v) && v == 10.0);
    CHECK(finish_accumulator(QE_AGG_SUM, 1, bits_of(-0.0), v) && bits_of(v) == bits_of(-0.0));
    CHECK(finish_accumulator(QE_AGG_AVG, 4, bits_of(10.0), v) && v == 2.5);                // AVG divides by the count
    CHECK(finish_accumulator(QE_AGG_AVG, 3, bits_of(1.0), v) && v == 1.0 / 3.0);
    // MIN / MAX round-trip through the ordered key, bit for bit
    const uint64_t specials[] = {bits_of(-kInf), bits_of(-1.5), bits_of(-0.0), bits_of(0.0), bits_of(5e-324), bits_of(kInf), kNaNBits};
    const int minmax[] = {QE_AGG_MIN, QE_AGG_MAX};
    for (uint64_t b : specials)
        for (int fn : minmax) {
            v = -1.0;
            CHECK(finish_accumulator(fn, 1, ordered_key(double_of(b)), v) && bits_of(v) == b);
        }
    CHECK((int64_t)ordered_key(-0.0) < (int64_t)ordered_key(0.0));                         // -0.0 orders below +0.0 in key space
    CHECK((int64_t)ordered_key(-kInf) < (int64_t)ordered_key(-1.5) && (int64_t)ordered_key(-1.5) < (int64_t)ordered_key(-0.0));
    CHECK((int64_t)ordered_key(0.0) < (int64_t)ordered_key(5e-324) && (int64_t)ordered_key(5e-324) < (int64_t)ordered_key(kInf));
}

static void test_aggregate_images() {
    // two groups x {first row, (count, acc) x 3}: aggregates 0 = SUM(x), 1 = AVG(x) sharing aggregate 0's counter, 2 = MIN(y).
    // Aggregate 1's OWN count word holds a decoy that a reader ignoring cnt_src would pick up.
    const uint64_t e[2][7] = {{0, 4, bits_of(10.0), 99, bits_of(10.0), 2, ordered_key(-0.0)},
                              {1, 0, bits_of(0.0), 99, bits_of(0.0), 0, agg_identity(QE_AGG_MIN)}};
    auto entry_of = [&](int64_t j) { return e[j]; };
    ColumnImage avg = aggregate_column_image(QE_AGG_AVG, 1, 0, 2, entry_of);
    CHECK(avg.w64.size() == 2 && avg.w64[0] == bits_of(2.5) && avg.w64[1] == bits_of(0.0));   // 10 / 4, not 10 / 99; NULL, not 0 / 99
    CHECK(avg.any_null && avg.valid.size() == 1 && avg.valid[0] == 1ull && avg.validity() == avg.valid.data());
    ColumnImage own = aggregate_column_image(QE_AGG_AVG, 1, 1, 2, entry_of);                 // (the decoy, when asked for)
    CHECK(own.w64[0] == bits_of(10.0 / 99) && !own.any_null && own.validity() == nullptr);
    ColumnImage mn = aggregate_column_image(QE_AGG_MIN, 2, 2, 2, entry_of);
    CHECK(mn.w64[0] == bits_of(-0.0) && mn.w64[1] == 0 && mn.any_null && mn.valid[0] == 1ull);
    ColumnImage cnt = aggregate_column_image(QE_AGG_COUNT, 0, 0, 2, entry_of);
    CHECK(cnt.w64[0] == bits_of(4.0) && cnt.w64[1] == bits_of(0.0) && !cnt.any_null && cnt.valid[0] == 3ull);
    ColumnImage none = aggregate_column_image(QE_AGG_SUM, 0, 0, 0, entry_of);                // no group: one spare value, one word
    CHECK(none.w64.size() == 1 && none.valid.size() == 1 && !none.any_null);
}

static void test_key_images() {
    const uint64_t words[] = {kNaNBits, bits_of(-0.0), 0xFFFFFFFFFFFFFFFFull, 1, 0};
    auto key_of = [&](int64_t j, uint64_t &w) { w = words[j]; return true; };
    ColumnImage d = key_column_image(QE_DOUBLE, 3, key_of);                                  // a DOUBLE key keeps its bits
    CHECK(d.w32.empty() && d.w64.size() == 3 && d.w64[0] == kNaNBits && d.w64[1] == bits_of(-0.0) && d.values() == d.w64.data());
    CHECK(!d.any_null && d.validity() == nullptr && d.valid[0] == 7ull);                     // no NULL: no bitmap goes out
    ColumnImage i64 = key_column_image(QE_INT64, 3, key_of);                                 // an INT64 key passes through
    CHECK(i64.w64[2] == 0xFFFFFFFFFFFFFFFFull && (int64_t)i64.w64[2] == -1);
    ColumnImage i32 = key_column_image(QE_INT32, 5, key_of);                                 // an INT32 key word of all ones is -1
    CHECK(i32.w64.empty() && i32.w32.size() == 5 && i32.w32[2] == -1 && i32.w32[3] == 1 && i32.values() == i32.w32.data());
    ColumnImage str = key_column_image(QE_STRING, 5, key_of);                                // dictionary codes: 4 bytes too
    CHECK(str.w32.size() == 5 && str.w32[3] == 1 && str.w32[4] == 0);
    // a NULL bit clears validity and leaves value 0 -- whatever word the accessor left
    auto with_null = [&](int64_t j, uint64_t &w) { w = 77; return j != 1; };
    ColumnImage n64 = key_column_image(QE_INT64, 3, with_null);
    CHECK(n64.any_null && n64.valid[0] == 5ull && n64.w64[0] == 77 && n64.w64[1] == 0 && n64.w64[2] == 77 && n64.validity() == n64.valid.data());
    ColumnImage n32 = key_column_image(QE_INT32, 3, with_null);
    CHECK(n32.any_null && n32.valid[0] == 5ull && n32.w32[1] == 0 && n32.w32[2] == 77);
    // m = 0, 1, 64, 65 rows across the word edge: BOOLEAN keys become bitmap words; row j is true when j % 3 == 0, NULL when j == 63
    for (int64_t m : {0, 1, 64, 65}) {
        auto bool_of = [&](int64_t j, uint64_t &w) { w = j % 3 == 0; return j != 63; };
        ColumnImage b = key_column_image(QE_BOOLEAN, m, bool_of);
        const size_t words_m = m <= 64 ? 1 : 2;
        CHECK(b.w32.empty() && b.w64.size() == words_m && b.valid.size() == words_m && b.any_null == (m >= 64));
        uint64_t want_bits[2] = {0, 0}, want_valid[2] = {0, 0};
        for (int64_t j = 0; j < m; j++) {
            if (j != 63) want_valid[j >> 6] |= 1ull << (j & 63);
            if (j != 63 && j % 3 == 0) want_bits[j >> 6] |= 1ull << (j & 63);
        }
        for (size_t w = 0; w < words_m; w++) CHECK(b.w64[w] == want_bits[w] && b.valid[w] == want_valid[w]);
        ColumnImage v = key_column_image(QE_INT64, m, [&](int64_t j, uint64_t &w) { w = (uint64_t)j + 1; return j != 63; });
        CHECK(v.w64.size() == (size_t)(m ? m : 1) && v.valid.size() == words_m && v.any_null == (m >= 64));
        for (int64_t j = 0; j < m; j++) CHECK(v.w64[j] == (j == 63 ? 0 : (uint64_t)j + 1));
        for (size_t w = 0; w < words_m; w++) CHECK(v.valid[w] == want_valid[w]);
    }
    ColumnImage b64 = key_column_image(QE_BOOLEAN, 64, [](int64_t j, uint64_t &w) { w = j % 3 == 0; return j != 63; });   // (written out)
    CHECK(b64.w64[0] == 0x1249249249249249ull && b64.valid[0] == 0x7FFFFFFFFFFFFFFFull);
    // the dense decode: key 0 of domain 3 (codes 0..2, 3 = NULL) has stride 1, key 1 of domain 2 (codes 0..1, 2 = NULL) stride 4
    const int want0[12] = {0, 1, 2, -1, 0, 1, 2, -1, 0, 1, 2, -1}, want1[12] = {0, 0, 0, 0, 1, 1, 1, 1, -1, -1, -1, -1};
    for (int64_t g = 0; g < 12; g++) {
        uint64_t w0 = 99, w1 = 99;
        const bool ok0 = dense_key_code(g, 1, 3, w0), ok1 = dense_key_code(g, 4, 2, w1);
        CHECK(ok0 == (want0[g] >= 0) && (!ok0 || w0 == (uint64_t)want0[g]));
        CHECK(ok1 == (want1[g] >= 0) && (!ok1 || w1 == (uint64_t)want1[g]));
    }
    ColumnImage k1 = key_column_image(QE_BOOLEAN, 12, [](int64_t g, uint64_t &w) { return dense_key_code(g, 4, 2, w); });
    CHECK(k1.w64[0] == 0x0F0ull && k1.valid[0] == 0x0FFull && k1.any_null);
    ColumnImage k0 = key_column_image(QE_STRING, 12, [](int64_t g, uint64_t &w) { return dense_key_code(g, 1, 3, w); });
    CHECK(k0.valid[0] == 0x777ull && k0.w32[2] == 2 && k0.w32[3] == 0 && k0.w32[6] == 2);
}

// m entries of `stride` words; entry g's first row is a fixed permutation of 0..m-1 (g * 7919 mod m, 7919 prime and no factor
// of any m used) times `scale`; `empty_every` > 0 leaves every such entry untouched (~0); `planted` replaces two values
static void order_case(int64_t m, uint64_t scale, int empty_every, bool planted) {
    const size_t stride = 3;
    std::vector<uint64_t> tab((size_t)std::max<int64_t>(m, 1) * stride, 0xABCDull);
    std::vector<std::pair<uint64_t, int64_t>> want;
    for (int64_t g = 0; g < m; g++) {
        uint64_t first = (uint64_t)((g * 7919) % m) * scale;
        if (planted && g == 5) first = (1ull << 42) - 1;      // the largest row id a batch can hold
        if (planted && g == 6) first = (1ull << 28) + 3;
        if (empty_every > 0 && g % empty_every == 2) first = ~0ull;
        tab[(size_t)g * stride] = first;
        if (first != ~0ull) want.emplace_back(first, g);
    }
    std::sort(want.begin(), want.end());
    const std::vector<int64_t> got = insertion_order(tab.data(), stride, m);
    CHECK(got.size() == want.size());
    for (size_t j = 0; j < got.size() && j < want.size(); j++)
        if (got[j] != want[j].second) {
            std::printf("FAIL insertion_order(m = %lld, scale %llu, empty every %d): position %zu is entry %lld, std::sort says %lld\n",
                        (long long)m, (unsigned long long)scale, empty_every, j, (long long)got[j], (long long)want[j].second);
            failures++;
            break;
        }
}

static void test_insertion_order() {
    for (int64_t m : {0, 1, 4095, 4096, 10000}) {
        order_case(m, 1, 0, false);                  // values < 2^14: from 4096 entries on ONE radix pass, the higher digits are skipped
        order_case(m, 1, 7, false);                  // with empty entries (4096 entries then hold fewer than 4096 groups: std::sort)
        order_case(m, 40000, 0, m > 6);              // values up to 4 * 10^8 >= 2^28, one 2^42 - 1: three passes, then no higher bits
        order_case(m, 40000, 5, m > 6);
        order_case(m, 1ull << 50, 0, false);         // (beyond any row id) bits up to 2^63: all five passes, no early exit
    }
    order_case(10000, 3, 0, false);                  // values < 2^28: two passes
}

static void test_global_fold() {
    const double nan = double_of(kNaNBits);
    // 3 workgroups x {(acc, count) x 5, selected rows}: MIN, MAX, SUM, COUNT, AVG
    const int32_t fns[5] = {QE_AGG_MIN, QE_AGG_MAX, QE_AGG_SUM, QE_AGG_COUNT, QE_AGG_AVG};
    double out[5];
    uint8_t valid[5];
    {
        const double p[3][11] = {{1.0, 2, 9.0, 2, 1.5, 2, 0.0, 3, 6.0, 2, 5},
                                 {nan, 1, nan, 1, 2.5, 1, 0.0, 4, 3.0, 1, 7},      // a NaN in the middle partial wins MIN and MAX
                                 {-3.0, 2, 11.0, 2, 4.0, 2, 0.0, 0, 1.0, 1, 11}};
        CHECK(fold_global_partials(&p[0][0], 3, fns, 5, out, valid) == 23);          // the selected-rows word sums
        CHECK(out[0] != out[0] && out[1] != out[1] && valid[0] == 1 && valid[1] == 1);
        CHECK(out[2] == 8.0 && valid[2] == 1);
        CHECK(out[3] == 7.0 && valid[3] == 1);                                       // COUNT sums
        CHECK(out[4] == 2.5 && valid[4] == 1);                                       // AVG = sum / count = 10 / 4
        CHECK(fold_global_partials(&p[0][0], 1, fns, 5, out, valid) == 5 && out[0] == 1.0 && out[1] == 9.0 && out[4] == 3.0);
    }
    {
        const double a[2][11] = {{-0.0, 1, -0.0, 1, 0, 0, 0, 0, 0, 0, 0}, {0.0, 1, 0.0, 1, 0, 0, 0, 0, 0, 0, 0}};
        const double b[2][11] = {{0.0, 1, 0.0, 1, 0, 0, 0, 0, 0, 0, 0}, {-0.0, 1, -0.0, 1, 0, 0, 0, 0, 0, 0, 0}};
        for (const double *p : {&a[0][0], &b[0][0]}) {                               // {-0.0, +0.0} in either order
            fold_global_partials(p, 2, fns, 5, out, valid);
            CHECK(bits_of(out[0]) == bits_of(-0.0) && bits_of(out[1]) == bits_of(0.0) && valid[0] == 1 && valid[1] == 1);
        }
    }
    {
        // all counts 0 (the accumulators as the kernel leaves them when no row is kept): NULL with 0.0; COUNT 0, valid
        const double p[2][11] = {{kInf, 0, -kInf, 0, 0.0, 0, 0.0, 0, 0.0, 0, 0}, {kInf, 0, -kInf, 0, 0.0, 0, 0.0, 0, 0.0, 0, 0}};
        for (int i = 0; i < 5; i++) { out[i] = -1.0; valid[i] = 9; }
        CHECK(fold_global_partials(&p[0][0], 2, fns, 5, out, valid) == 0);
        for (int i = 0; i < 5; i++) CHECK(bits_of(out[i]) == bits_of(0.0) && valid[i] == (i == 3 ? 1 : 0));
        for (int i = 0; i < 5; i++) { out[i] = -1.0; valid[i] = 9; }
        CHECK(fold_global_partials(nullptr, 0, fns, 5, out, valid) == 0);            // an empty batch: no workgroup ran
        for (int i = 0; i < 5; i++) CHECK(bits_of(out[i]) == bits_of(0.0) && valid[i] == (i == 3 ? 1 : 0));
    }
}

int main() {
    test_identity_and_finish();
    test_aggregate_images();
    test_key_images();
    test_insertion_order();
    test_global_fold();
    if (failures) {
        std::printf("%d group finish checks FAILED\n", failures);
        return 1;
    }
    std::printf("all group finish checks passed\n");
    return 0;
}
