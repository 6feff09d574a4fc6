// qe_group_finish.cpp -- the parts of qe_group_finish.h that are no templates: insertion order and the global aggregate's fold.
#include "qe_group_finish.h"

#include <cmath>
#include <utility>

namespace qe {

std::vector<int64_t> insertion_order(const uint64_t *first_row, size_t stride, int64_t m) {
    std::vector<std::pair<uint64_t, int64_t>> order;
    order.reserve((size_t)m);
    for (int64_t g = 0; g < m; g++)
        if (first_row[(size_t)g * stride] != ~0ull) order.emplace_back(first_row[(size_t)g * stride], g);
    if (order.size() < 4096) {
        std::sort(order.begin(), order.end());
    } else {
        // three passes for row ids < 2^42; a pass whose digit and every higher one are 0 everywhere is not run (std::sort took
        // ~80 of the 125 ms the host spent finishing 1 M groups)
        std::vector<std::pair<uint64_t, int64_t>> tmp(order.size());
        std::vector<size_t> cnt((size_t)1 << 14);
        uint64_t all = 0;
        for (const auto &o : order) all |= o.first;
        for (int pass = 0; pass < 5 && (all >> (14 * pass)) != 0; pass++) {
            const int sh = 14 * pass;
            std::fill(cnt.begin(), cnt.end(), 0);
            for (const auto &o : order) cnt[(size_t)((o.first >> sh) & 0x3fffull)]++;
            size_t run = 0;
            for (size_t &c : cnt) { const size_t t = c; c = run; run += t; }
            for (const auto &o : order) tmp[cnt[(size_t)((o.first >> sh) & 0x3fffull)]++] = o;
            order.swap(tmp);
        }
    }
    std::vector<int64_t> entries(order.size());
    for (size_t j = 0; j < order.size(); j++) entries[j] = order[j].second;
    return entries;
}

int64_t fold_global_partials(const double *partial, int nworkgroups, const int32_t *agg_fns, int nagg, double *out_values, uint8_t *out_valid) {
    const size_t stride = 2 * (size_t)nagg + 1;
    for (int i = 0; i < nagg; i++) {
        const int fn = agg_fns[i];
        double acc = fn == QE_AGG_MIN ? INFINITY : fn == QE_AGG_MAX ? -INFINITY : 0.0;
        double cnt = 0;
        for (int b = 0; b < nworkgroups; b++) {
            const double a = partial[(size_t)b * stride + 2 * i], c = partial[(size_t)b * stride + 2 * i + 1];
            cnt += c;
            if (fn == QE_AGG_MIN) acc = (a != a || acc != acc) ? (acc != acc ? acc : a)
                                      : (a == 0.0 && acc == 0.0 ? (std::signbit(acc) ? acc : a) : std::min(acc, a));
            else if (fn == QE_AGG_MAX) acc = (a != a || acc != acc) ? (acc != acc ? acc : a)
                                           : (a == 0.0 && acc == 0.0 ? (std::signbit(acc) ? a : acc) : std::max(acc, a));
            else acc += a;
        }
        out_valid[i] = fn == QE_AGG_COUNT || cnt != 0;   // Accumulators.kt:26-36 a COUNT is never NULL, :47-53 empty => null
        out_values[i] = fn == QE_AGG_COUNT ? cnt : cnt == 0 ? 0.0 : fn == QE_AGG_AVG ? acc / cnt : acc;   // :101-107
    }
    int64_t nsel = 0;
    for (int b = 0; b < nworkgroups; b++) nsel += (int64_t)partial[(size_t)b * stride + 2 * nagg];
    return nsel;
}

}  // namespace qe
