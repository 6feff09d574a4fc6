// qe_group_finish.h -- how the accumulator words of a group become a result row, in ONE place: the identity of an empty
// accumulator, the finish rule (Accumulators.kt:26-107), insertion order, the host image of a result column, and the fold of the
// global aggregate's partials.  Host only, no HIP, nothing uploaded: qe_groupby.cpp feeds these with table entries and uploads
// what comes back; tests/group_finish_test.cpp feeds them by hand.  agg_identity and finish_accumulator also compile as device
// code: group_finish_kernel (qe_kernels.hip) finishes large results with the same switch.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/qe_hip.h"

#ifdef __HIPCC__
#define QE_HOST_DEVICE __host__ __device__
#else
#define QE_HOST_DEVICE
#endif

namespace qe {

// MIN / MAX accumulate the ORDERED KEY of a double, b ^ ((b >> 63) & 0x7fff..): signed integer order = Double.compare order
// (-0.0 below +0.0).  The accumulator word of an aggregate that has seen no value: the largest / smallest key, else 0 (= +0.0).
QE_HOST_DEVICE inline uint64_t agg_identity(int fn) { return fn == QE_AGG_MIN ? 0x7fffffffffffffffull : fn == QE_AGG_MAX ? 0x8000000000000000ull : 0ull; }

// Aggregate `fn` finished from its accumulator word `raw` and the `count` of values it saw; false = NULL, and value 0.0.
QE_HOST_DEVICE inline bool finish_accumulator(int fn, uint64_t count, uint64_t raw, double &value) {
    value = fn == QE_AGG_COUNT ? (double)count : 0.0;       // Accumulators.kt:26-36
    if (fn == QE_AGG_COUNT) return true;
    if (count == 0) return false;                            // :47-53 empty => null
    if (fn == QE_AGG_MIN || fn == QE_AGG_MAX) raw ^= (uint64_t)((int64_t)raw >> 63) & 0x7fffffffffffffffull;   // undo the ordered key
    __builtin_memcpy(&value, &raw, 8);
    if (fn == QE_AGG_AVG) value /= (double)count;            // :101-107
    return true;
}

// The entries of a table in insertion order = ascending first row (LinkedHashMap, GroupByAggregationOperator.kt:22).  Entry g's
// first row is first_row[g * stride]; ~0 marks an entry no row reached, which is left out.  First rows are distinct row ids
// < 2^42.  Below 4096 entries std::sort, from there stable passes of a 14-bit radix sort over the bits in use.
std::vector<int64_t> insertion_order(const uint64_t *first_row, size_t stride, int64_t m);

// One result column of m rows as the device wants it.  w64: 8-byte values as their bits (DOUBLE, INT64), or the bitmap words
// of a BOOLEAN column; w32: 4-byte values (INT32, dictionary codes).  A NULL row has value 0 and its bit in `valid` clear; a
// column with any_null == false goes out without a bitmap.
struct ColumnImage {
    std::vector<uint64_t> w64, valid;
    std::vector<int32_t> w32;
    bool any_null = false;
    const void *values() const { return w32.empty() ? (const void *)w64.data() : (const void *)w32.data(); }
    const uint64_t *validity() const { return any_null ? valid.data() : nullptr; }
};

// A key column of type `type`: key_of(j, word) is false for a NULL, else leaves row j's key as a 64-bit word -- the canonical
// bits of a DOUBLE, the value of an INT64, the (sign-extended) INT32 or dictionary code, 0 / 1 of a BOOLEAN.
template <typename KeyOf>
ColumnImage key_column_image(int type, int64_t m, KeyOf key_of) {
    ColumnImage c;
    const size_t rows = (size_t)std::max<int64_t>(m, 1), words = (size_t)std::max<int64_t>(1, (m + 63) / 64);
    const bool bits = type == QE_BOOLEAN, wide = type == QE_DOUBLE || type == QE_INT64;
    c.valid.assign(words, 0);
    if (bits || wide) c.w64.assign(bits ? words : rows, 0);
    else c.w32.assign(rows, 0);
    for (int64_t j = 0; j < m; j++) {
        uint64_t kw = 0;
        if (!key_of(j, kw)) { c.any_null = true; continue; }
        c.valid[j >> 6] |= 1ull << (j & 63);
        if (bits) c.w64[j >> 6] |= (uint64_t)(kw != 0) << (j & 63);
        else if (wide) c.w64[j] = kw;
        else c.w32[j] = (int32_t)(int64_t)kw;
    }
    return c;
}

// Key k of a DENSE group id: the id is sum of code_k * stride_k, stride_k = product of (domain + 1) of the keys before k, and
// code == domain is the NULL key.
inline bool dense_key_code(int64_t group, int64_t stride, int domain, uint64_t &word) {
    word = (uint64_t)((group / stride) % (domain + 1));
    return word != (uint64_t)domain;
}

// Aggregate i (function `fn`) of m groups, a DOUBLE column: entry_of(j) = row j's words {first row, (count, acc) per
// aggregate}.  cnt_src: the aggregate whose counter says how many values aggregate i saw (aggregates over one input share it).
template <typename EntryOf>
ColumnImage aggregate_column_image(int fn, int i, int cnt_src, int64_t m, EntryOf entry_of) {
    ColumnImage c;
    c.w64.assign((size_t)std::max<int64_t>(m, 1), 0);
    c.valid.assign((size_t)std::max<int64_t>(1, (m + 63) / 64), 0);
    for (int64_t j = 0; j < m; j++) {
        const uint64_t *e = entry_of(j);
        double v;
        if (finish_accumulator(fn, e[1 + 2 * cnt_src], e[2 + 2 * i], v)) c.valid[j >> 6] |= 1ull << (j & 63);
        else c.any_null = true;
        __builtin_memcpy(&c.w64[j], &v, 8);
    }
    return c;
}

// The global aggregate: `partial` holds, per workgroup, {(acc, count) per aggregate.., selected rows} as doubles.  Folded in
// workgroup order (the grid is fixed, so the sum is reproducible) with Java's Math.min / Math.max: a NaN wins, -0.0 < +0.0.
// Returns the selected rows.
int64_t fold_global_partials(const double *partial, int nworkgroups, const int32_t *agg_fns, int nagg, double *out_values, uint8_t *out_valid);

}  // namespace qe
