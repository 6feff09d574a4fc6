// qe_csv_number.h -- java.lang.Double.parseDouble for the device CSV parser (qe_csv_device.hip), as __host__ __device__
// functions so that a host test can compile this header on its own and check it against strtod bit for bit.
//
// qe_parse_double(p, n, &out) decides a field in one of three ways:
//   QE_NUM_OK        the text is a Java floating literal and *out is its correctly rounded value (= strtod's);
//   QE_NUM_REJECT    Java rejects the text (NumberFormatException);
//   QE_NUM_UNDECIDED the grammar accepts it but this converter does not decide it: more than 19 significant digits, a
//                    hexadecimal literal, or an Eisel-Lemire product too close to a rounding boundary.  The caller hands
//                    such a field to the host converter (java_parse_double in qe_csv.cpp); it never guesses.
// The grammar is the one java_parse_double checks: bytes <= 0x20 trimmed at both ends, an optional sign, "NaN",
// "Infinity", a decimal literal (digits, optional '.', digits, optional e/E exponent) or a hexadecimal one (0x.., the p
// exponent mandatory), then an optional d/D/f/F suffix.
// Conversion: Clinger's fast path when the mantissa is below 2^53 and |exp10| <= 22 (one correctly rounded multiply or
// divide of two exact doubles), otherwise Eisel-Lemire (Lemire, "Number Parsing at a Gigabyte per Second", 2021) over the
// 128-bit powers of five of qe_pow5_table.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QE_HD __host__ __device__
#ifndef QE_POW5_STORAGE
#define QE_POW5_STORAGE static __device__ const
#endif
#else
#define QE_HD
#ifndef QE_POW5_STORAGE
#define QE_POW5_STORAGE static const
#endif
#endif

#include "qe_pow5_table.h"

enum { QE_NUM_OK = 0, QE_NUM_REJECT = 1, QE_NUM_UNDECIDED = 2 };

QE_HD inline double qe_bits_to_double(uint64_t b) {
    union { uint64_t u; double d; } x;
    x.u = b;
    return x.d;
}

QE_HD inline void qe_mul_64x64(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    hi = __umul64hi(a, b);
    lo = a * b;
#else
    const unsigned __int128 p = (unsigned __int128)a * b;
    hi = (uint64_t)(p >> 64);
    lo = (uint64_t)p;
#endif
}

QE_HD inline int qe_clz64(uint64_t x) {   // x != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// Eisel-Lemire: w * 10^q for w != 0 (at most 19 digits), q in [QE_POW5_QMIN, QE_POW5_QMAX].  Returns false when the
// truncated product cannot decide the rounding.
QE_HD inline bool qe_eisel_lemire(uint64_t w, int q, uint64_t &bits) {
    const int lz = qe_clz64(w);
    w <<= lz;
    const int idx = 2 * (q - QE_POW5_QMIN);
    uint64_t hi, lo;
    qe_mul_64x64(w, qe_pow5_128[idx], hi, lo);
    const uint64_t precision_mask = 0xFFFFFFFFFFFFFFFFull >> 55;   // 52 mantissa bits + 3
    if ((hi & precision_mask) == precision_mask) {   // the low half of the power may carry into the kept bits
        uint64_t hi2, lo2;
        qe_mul_64x64(w, qe_pow5_128[idx + 1], hi2, lo2);
        lo += hi2;
        if (hi2 > lo) hi++;
        if (lo == 0xFFFFFFFFFFFFFFFFull && (q < -27 || q > 55)) return false;   // still ambiguous: the host decides
    }
    const int upper = (int)(hi >> 63);
    uint64_t m = hi >> (upper + 9);
    int p2 = (int)(((152170 + 65536) * (int64_t)q) >> 16) + 63 + upper - lz + 1023;
    if (p2 <= 0) {   // subnormal (or zero)
        if (-p2 + 1 >= 64) { bits = 0; return true; }
        m >>= -p2 + 1;
        m += m & 1;
        m >>= 1;
        p2 = m < (1ull << 52) ? 0 : 1;
        bits = (m & ((1ull << 52) - 1)) | ((uint64_t)p2 << 52);
        return true;
    }
    // exactly halfway between two doubles: round to even (only possible for small |q|)
    if (lo <= 1 && q >= -4 && q <= 23 && (m & 3) == 1 && (m << (upper + 9)) == hi) m &= ~1ull;
    m += m & 1;
    m >>= 1;
    if (m >= (2ull << 52)) { m = 1ull << 52; p2++; }
    m &= ~(1ull << 52);
    if (p2 >= 0x7FF) { p2 = 0x7FF; m = 0; }
    bits = m | ((uint64_t)p2 << 52);
    return true;
}

QE_HD inline bool qe_is_digit(unsigned char c) { return c >= '0' && c <= '9'; }
QE_HD inline bool qe_is_xdigit(unsigned char c) { return qe_is_digit(c) || ((c | 0x20) >= 'a' && (c | 0x20) <= 'f'); }

QE_HD inline int qe_parse_double(const unsigned char *p, size_t n, double &out) {
    while (n > 0 && p[0] <= 0x20) { p++; n--; }
    while (n > 0 && p[n - 1] <= 0x20) n--;
    if (n == 0) return QE_NUM_REJECT;
    size_t i = 0;
    bool neg = false;
    if (p[0] == '+' || p[0] == '-') { neg = p[0] == '-'; i++; }
    const uint64_t sign = neg ? 0x8000000000000000ull : 0;
    const size_t m = n - i;
    const unsigned char *b = p + i;
    if (m == 3 && b[0] == 'N' && b[1] == 'a' && b[2] == 'N') { out = qe_bits_to_double(0x7ff8000000000000ull); return QE_NUM_OK; }
    if (m == 8 && b[0] == 'I' && b[1] == 'n' && b[2] == 'f' && b[3] == 'i' && b[4] == 'n' && b[5] == 'i' && b[6] == 't' && b[7] == 'y') {
        out = qe_bits_to_double(sign | 0x7ff0000000000000ull);
        return QE_NUM_OK;
    }
    size_t j = 0;
    if (m > 2 && b[0] == '0' && (b[1] == 'x' || b[1] == 'X')) {   // hexadecimal: grammar only, the host converts
        j = 2;
        size_t a = 0, f = 0;
        while (j < m && qe_is_xdigit(b[j])) { j++; a++; }
        if (j < m && b[j] == '.') { j++; while (j < m && qe_is_xdigit(b[j])) { j++; f++; } }
        if (a + f == 0) return QE_NUM_REJECT;
        if (j >= m || (b[j] | 0x20) != 'p') return QE_NUM_REJECT;
        j++;
        if (j < m && (b[j] == '+' || b[j] == '-')) j++;
        size_t e = 0;
        while (j < m && qe_is_digit(b[j])) { j++; e++; }
        if (e == 0) return QE_NUM_REJECT;
        if (j < m && (b[j] == 'd' || b[j] == 'D' || b[j] == 'f' || b[j] == 'F')) j++;
        return j == m ? QE_NUM_UNDECIDED : QE_NUM_REJECT;
    }
    // decimal: w = the significant digits (leading zeros skipped), q = the power of ten that scales them
    uint64_t w = 0;
    int sig = 0;            // significant digits taken into w (saturates at 20: "more than 19")
    int64_t q = 0;
    size_t a = 0, f = 0;
    while (j < m && qe_is_digit(b[j])) {
        const unsigned d = b[j] - '0';
        if (sig > 0 || d != 0) {
            if (sig < 19) w = w * 10 + d;
            else q++;   // a digit beyond the 19th (only matters for the grammar: the field is undecided below)
            if (sig < 20) sig++;
        }
        j++;
        a++;
    }
    if (j < m && b[j] == '.') {
        j++;
        while (j < m && qe_is_digit(b[j])) {
            const unsigned d = b[j] - '0';
            if (sig > 0 || d != 0) {
                if (sig < 19) { w = w * 10 + d; q--; }
                if (sig < 20) sig++;
            } else {
                q--;   // a leading zero after the point
            }
            j++;
            f++;
        }
    }
    if (a + f == 0) return QE_NUM_REJECT;
    if (j < m && (b[j] == 'e' || b[j] == 'E')) {
        j++;
        bool eneg = false;
        if (j < m && (b[j] == '+' || b[j] == '-')) { eneg = b[j] == '-'; j++; }
        size_t e = 0;
        int64_t ev = 0;
        while (j < m && qe_is_digit(b[j])) {
            if (ev < 100000000) ev = ev * 10 + (b[j] - '0');   // saturates far outside the range of a double
            j++;
            e++;
        }
        if (e == 0) return QE_NUM_REJECT;
        q += eneg ? -ev : ev;
    }
    if (j < m && (b[j] == 'd' || b[j] == 'D' || b[j] == 'f' || b[j] == 'F')) j++;
    if (j != m) return QE_NUM_REJECT;
    if (sig > 19) return QE_NUM_UNDECIDED;
    if (w == 0) { out = qe_bits_to_double(sign); return QE_NUM_OK; }
    if (q < QE_POW5_QMIN) { out = qe_bits_to_double(sign); return QE_NUM_OK; }                          // < 10^-323: zero
    if (q > QE_POW5_QMAX) { out = qe_bits_to_double(sign | 0x7ff0000000000000ull); return QE_NUM_OK; }  // >= 10^309: inf
    if (w < (1ull << 53) && q >= -22 && q <= 22) {   // Clinger: both operands exact, one correctly rounded operation
        const double pow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
        double v = (double)w;
        v = q < 0 ? v / pow10[-q] : v * pow10[q];
        out = neg ? -v : v;
        return QE_NUM_OK;
    }
    uint64_t bits;
    if (!qe_eisel_lemire(w, (int)q, bits)) return QE_NUM_UNDECIDED;
    out = qe_bits_to_double(sign | bits);
    return QE_NUM_OK;
}
