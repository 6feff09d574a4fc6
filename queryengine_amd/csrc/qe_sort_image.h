// qe_sort_image.h -- device code: the order-preserving u64 image of one value of a key column, as the ORDER BY kernels
// (qe_sort.hip) and the boundary flags of the window operator (qe_window.hip) both take it -- two rows the sort saw as equal
// on a key are equal for the flags by construction.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/qe_hip.h"

namespace qe {

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32;

__device__ __forceinline__ bool bit_at(const u64 *bm, i64 i) { return (bm[i >> 6] >> (i & 63)) & 1ull; }

// image of row i: unsigned order = compareValues order of the values; 0 under a NULL (validity is kept beside the image)
__device__ __forceinline__ u64 sort_image(int type, const void *data, const u64 *validity, const int *ranks, int nranks, i64 i) {
    u64 k = 0;   // NULL: before every value (compareValues)
    if (!validity || bit_at(validity, i)) {
        switch (type) {
        case QE_DOUBLE: {   // Double.compareTo: IEEE order with -0.0 < 0.0, every NaN equal and greatest
            const double d = ((const double *)data)[i];
            i64 b = d != d ? 0x7ff8000000000000ll : __builtin_bit_cast(i64, d);
            b ^= (b >> 63) & 0x7fffffffffffffffll;            // negative values: reverse their order
            k = ((u64)b ^ 0x8000000000000000ull);             // signed -> unsigned order
            break;
        }
        case QE_INT64: k = (u64)((const i64 *)data)[i] ^ 0x8000000000000000ull; break;
        case QE_INT32: k = (u64)(i64)((const int *)data)[i] ^ 0x8000000000000000ull; break;
        case QE_STRING: {   // rank of the code in the dictionary's String.compareTo order (table from the host)
            const int c = ((const int *)data)[i];
            k = (u64)((u32)c < (u32)nranks ? ranks[c] : 0);
            break;
        }
        default: k = bit_at((const u64 *)data, i) ? 1ull : 0ull; break;   // BOOLEAN bitmap
        }
    }
    return k;
}

}  // namespace qe
