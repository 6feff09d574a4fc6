// qe_pernode_kernels.hip -- one precompiled gfx950 kernel per expression node kind
// (SURVEY 2.1 kernel inventory): arithmetic, negate, ABS / FLOOR / CEIL, cast, comparison -> bitmap via
// __ballot, Kleene logic on 64-row words, IF select, and the gather behind the
// filter's stable compaction (bitmap_ranks -> bitmap_positions of qe_scan.h -> gather).
//
// Semantics per node follow evaluator/Interpreter.kt:94-107 (JVM DADD..DREM,
// Double.compare / equals) exactly as the fused kernels do; validity is handled
// by the executor with word-parallel bitmap kernels (k = ka & kb etc.).
//
// Four kernels are written out, the measured ones: k_arith, k_cmp, k_cmp_rows, k_gather_multi.  Every other node is a one-line
// functor under k_map (a grid-stride loop over rows or words) or k_ballot (the same loop, 64 results -> one bitmap word).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <type_traits>

#include "qe_pernode_kernels.h"
#include "../../include/qe_hip.h"

namespace qe {
namespace pn {

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32;

template <typename T> struct Ld {
    const T *p;
    T s;
    const u32 *idx;   // selection vector (Opnd::idx) or null
    __device__ __forceinline__ T operator[](i64 i) const { return p ? (idx ? p[idx[i]] : p[i]) : s; }
};

template <typename T> static Ld<T> mk(const Opnd &o);
template <> Ld<double> mk<double>(const Opnd &o) { return Ld<double>{(const double *)o.ptr, o.f, o.idx}; }
template <> Ld<i64> mk<i64>(const Opnd &o) { return Ld<i64>{(const i64 *)o.ptr, (i64)o.i, o.idx}; }
template <> Ld<int> mk<int>(const Opnd &o) { return Ld<int>{(const int *)o.ptr, (int)o.i, o.idx}; }

static inline int grid_for(int64_t n, int per_block = 256, int cap = 16384) {
    int64_t b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- runtime type / operator -> compile-time -------------------------------------------------------------------------
// with_type(type, f): f(Tag<T>) with T the element type of the QE_* code: double, i64, or int (INT32, dictionary codes)
template <typename T> struct Tag { typedef T type; };
template <typename F> static void with_type(int type, F f) {
    if (type == QE_DOUBLE) f(Tag<double>{});
    else if (type == QE_INT64) f(Tag<i64>{});
    else f(Tag<int>{});
}
#define QE_TAG_TYPE(t) typename decltype(t)::type

// with_const<N>(v, f): f(Const<v>) for an Arith / Unary / Cmp value v in 0 .. N - 1 (anything else takes the last one)
template <int V> struct Const { static constexpr int value = V; };
template <int N, int V = 0, typename F> static void with_const(int v, F f) {
    if constexpr (V + 1 == N) f(Const<V>{});
    else if (v == V) f(Const<V>{});
    else with_const<N, V + 1>(v, f);
}

// ---- the two loops every small node shares -------------------------------------------------------------------------
// f(i) for every i < n; f is a small functor passed by value (its pointers and scalars arrive as kernel arguments)
template <typename F> __global__ void __launch_bounds__(256) k_map(F f, i64 n) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) f(i);
}
template <typename F> static void map(hipStream_t s, int64_t n, F f) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_map<F>, dim3(grid_for(n)), dim3(256), 0, s, f, (i64)n);
}

// bit i of `out` = test(i), one __ballot per 64 rows; the loop runs over the rows padded to whole words so that every lane of
// the last word's wave takes part: bits of rows >= n are 0.  test is the functor itself, unless it has a row_test of its own
// (MemberHashFn: the set's header, read once per lane in front of the loop -- inside it the header would be read again on
// every trip, since the stores to `out` may alias it)
template <typename F> __device__ __forceinline__ const F &row_test(const F &f) { return f; }
template <typename F> __global__ void __launch_bounds__(256) k_ballot(F f, u64 *out, i64 n) {
    const auto &test = row_test(f);
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const i64 padded = (n + 63) & ~63ll;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        const bool r = i < n && test(i);
        const u64 w = __ballot(r);
        if ((threadIdx.x & 63) == 0) out[i >> 6] = w;
    }
}
template <typename F> static void ballot(hipStream_t s, int64_t n, uint64_t *out, F f) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_ballot<F>, dim3(grid_for(n)), dim3(256), 0, s, f, (u64 *)out, (i64)n);
}

// ---- arithmetic ------------------------------------------------------------------------------------
template <typename T, int OP> struct ArithOp;
template <int OP> struct ArithOp<double, OP> {
    static __device__ __forceinline__ double apply(double a, double b) {
        if (OP == A_ADD) return a + b;
        if (OP == A_SUB) return a - b;
        if (OP == A_MUL) return a * b;
        if (OP == A_DIV) return a / b;
        return fmod(a, b);   // DREM
    }
};
template <int OP> struct ArithOp<i64, OP> {
    static __device__ __forceinline__ i64 apply(i64 a, i64 b) {
        if (OP == A_ADD) return (i64)((u64)a + (u64)b);
        if (OP == A_SUB) return (i64)((u64)a - (u64)b);
        if (OP == A_MUL) return (i64)((u64)a * (u64)b);
        const i64 d = b == 0 ? 1 : b;   // row is NULL anyway (nonzero bitmap)
        if (OP == A_DIV) return d == -1 ? (i64)(0ull - (u64)a) : a / d;
        return d == -1 ? 0 : a % d;
    }
};
template <int OP> struct ArithOp<int, OP> {
    static __device__ __forceinline__ int apply(int a, int b) {
        if (OP == A_ADD) return (int)((u32)a + (u32)b);
        if (OP == A_SUB) return (int)((u32)a - (u32)b);
        if (OP == A_MUL) return (int)((u32)a * (u32)b);
        const int d = b == 0 ? 1 : b;
        if (OP == A_DIV) return d == -1 ? (int)(0u - (u32)a) : a / d;
        return d == -1 ? 0 : a % d;
    }
};

// Two rows per lane and load: 16 bytes for the 8-byte types (global_load_dwordx4, 1 KiB contiguous per wave instruction),
// 4 pairs in flight per lane before the first use; a scalar operand lives in SGPRs (no column of copies).
template <typename T> struct Pair { T x, y; };
template <typename T> struct V2;
template <> struct V2<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct V2<i64> { typedef i64 type __attribute__((ext_vector_type(2))); };
template <> struct V2<int> { typedef int type __attribute__((ext_vector_type(2))); };
template <typename T> using Vec2 = typename V2<T>::type;

template <typename T> __device__ __forceinline__ Pair<T> ld2(const Ld<T> &a, i64 pair) {
    if (!a.p) return Pair<T>{a.s, a.s};
    if (a.idx) {   // through the selection vector: the two row ids in one 8-byte load, then two gathers
        typedef u32 U2 __attribute__((ext_vector_type(2)));
        const U2 r = __builtin_nontemporal_load((const U2 *)a.idx + pair);
        return Pair<T>{a.p[r.x], a.p[r.y]};
    }
    const Vec2<T> v = __builtin_nontemporal_load((const Vec2<T> *)a.p + pair);
    return Pair<T>{v.x, v.y};
}

template <typename T, int OP>
__global__ void __launch_bounds__(256) k_arith(Ld<T> a, Ld<T> b, T *out, i64 n) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const i64 npairs = n >> 1;
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < npairs; i += 4 * stride) {
        Pair<T> x[4], y[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { x[j] = ld2(a, i + j * stride); y[j] = ld2(b, i + j * stride); }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            Vec2<T> r;
            r.x = ArithOp<T, OP>::apply(x[j].x, y[j].x);
            r.y = ArithOp<T, OP>::apply(x[j].y, y[j].y);
            ((Vec2<T> *)out)[i + j * stride] = r;
        }
    }
    for (; i < npairs; i += stride) {
        const Pair<T> x = ld2(a, i), y = ld2(b, i);
        Vec2<T> r;
        r.x = ArithOp<T, OP>::apply(x.x, y.x);
        r.y = ArithOp<T, OP>::apply(x.y, y.y);
        ((Vec2<T> *)out)[i] = r;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = ArithOp<T, OP>::apply(a[n - 1], b[n - 1]);
}

void arith(hipStream_t s, int type, int op, Opnd a, Opnd b, void *out, int64_t n) {
    if (n <= 0) return;
    const int g = grid_for((n + 1) / 2, 256, 256 * 8);
    with_type(type, [&](auto t) {
        typedef QE_TAG_TYPE(t) T;
        with_const<A_MOD + 1>(op, [&](auto c) {
            hipLaunchKernelGGL((k_arith<T, decltype(c)::value>), dim3(g), dim3(256), 0, s, mk<T>(a), mk<T>(b), (T *)out, (i64)n);
        });
    });
}

// ---- elementwise: negate, ABS / FLOOR / CEIL, cast, literal fill -------------------------------------------------------
// DNEG / LNEG / INEG.  ABS / FLOOR / CEIL (extensions): Math.abs clears the sign bit (-0.0 -> 0.0, NaN stays NaN) and wraps at
// long / int MIN_VALUE; Math.floor / Math.ceil are the IEEE roundings (ceil(-0.5) = -0.0).  The executor never launches
// FLOOR / CEIL on integers.
template <typename T, int OP> struct UnaryOp {   // i64 / int
    static __device__ __forceinline__ T apply(T a) {
        typedef typename std::make_unsigned<T>::type U;
        return OP == U_NEG || (OP == U_ABS && a < 0) ? (T)((U)0 - (U)a) : a;
    }
};
template <int OP> struct UnaryOp<double, OP> {
    static __device__ __forceinline__ double apply(double a) {
        if (OP == U_NEG) return -a;
        if (OP == U_ABS) return __builtin_fabs(a);
        if (OP == U_FLOOR) return floor(a);
        return ceil(a);
    }
};
template <typename T, int OP> struct UnaryFn {
    const T *a;
    T *out;
    __device__ void operator()(i64 i) const { out[i] = UnaryOp<T, OP>::apply(a[i]); }
};
void unary(hipStream_t s, int type, int op, const void *a, void *out, int64_t n) {
    with_type(type, [&](auto t) {
        typedef QE_TAG_TYPE(t) T;
        with_const<U_NEG + 1>(op, [&](auto c) { map(s, n, UnaryFn<T, decltype(c)::value>{(const T *)a, (T *)out}); });
    });
}

template <typename F, typename T> struct CastFn {
    const F *a;
    T *out;
    __device__ void operator()(i64 i) const { out[i] = (T)a[i]; }
};
void cast(hipStream_t s, int from, int to, const void *a, void *out, int64_t n) {
    if (from == QE_INT64 && to == QE_DOUBLE) map(s, n, CastFn<i64, double>{(const i64 *)a, (double *)out});
    else if (from == QE_INT32 && to == QE_DOUBLE) map(s, n, CastFn<int, double>{(const int *)a, (double *)out});
    else map(s, n, CastFn<int, i64>{(const int *)a, (i64 *)out});
}

template <typename T> struct FillFn {
    T v;
    T *out;
    __device__ void operator()(i64 i) const { out[i] = v; }
};
void fill(hipStream_t s, int type, Opnd v, void *out, int64_t n) {
    with_type(type, [&](auto t) {
        typedef QE_TAG_TYPE(t) T;
        map(s, n, FillFn<T>{mk<T>(v).s, (T *)out});
    });
}

// ---- comparison -> bitmap -----------------------------------------------------------------------------
__device__ __forceinline__ i64 canon_bits(double d) { return d != d ? 0x7ff8000000000000ll : __builtin_bit_cast(i64, d); }
__device__ __forceinline__ int dcmp(double a, double b) {   // java.lang.Double.compare
    if (a < b) return -1;
    if (a > b) return 1;
    const i64 x = canon_bits(a), y = canon_bits(b);
    return x == y ? 0 : (x < y ? -1 : 1);
}

template <typename T, int CMP, int IEEE> struct CmpOp {
    static __device__ __forceinline__ bool apply(T a, T b) {
        if (CMP == C_LT) return a < b;
        if (CMP == C_LE) return a <= b;
        if (CMP == C_GE) return a >= b;
        if (CMP == C_GT) return a > b;
        if (CMP == C_EQ) return a == b;
        return a != b;
    }
};
template <int CMP> struct CmpOp<double, CMP, 0> {   // total order: INTERPRETER / BYTECODE_COMPILER
    static __device__ __forceinline__ bool apply(double a, double b) {
        if (CMP == C_EQ) return canon_bits(a) == canon_bits(b);
        if (CMP == C_NE) return canon_bits(a) != canon_bits(b);
        const int c = dcmp(a, b);
        if (CMP == C_LT) return c < 0;
        if (CMP == C_LE) return c <= 0;
        if (CMP == C_GE) return c >= 0;
        return c > 0;
    }
};
template <int CMP> struct CmpOp<double, CMP, 1> {   // CLOSURE_COMPILER: IEEE <,<=,>=,>; equals() for ==, !=
    static __device__ __forceinline__ bool apply(double a, double b) {
        if (CMP == C_EQ) return canon_bits(a) == canon_bits(b);
        if (CMP == C_NE) return canon_bits(a) != canon_bits(b);
        if (CMP == C_LT) return a < b;
        if (CMP == C_LE) return a <= b;
        if (CMP == C_GE) return a >= b;
        return a > b;
    }
};

// A wave handles chunks of 4 adjacent groups of 128 rows (4 KiB of an 8-byte column): lane l loads rows 2l, 2l+1 of each
// group with ONE load (16 bytes for the 8-byte types, 1 KiB contiguous per wave instruction), all 4 in flight before the
// first use.  Lane l holds the results of rows 2l, 2l+1; word 0 of a group (rows 0..63) wants row i in bit i: lane i fetches
// the pair of lane i >> 1 (word 1: lane 32 + (i >> 1)) with a cross-lane permute and ballots its bit i & 1.  The chunk's 8
// result words leave in ONE store instruction (lanes 0..7, 64 contiguous bytes): a store per word from a single lane kept
// the address unit busy for a whole wave instruction each (15.6 M of them per 1 B rows: 1.6 - 1.9 ms per 8 GB column
// instead of 1.3), and so did interleaving the even / odd ballots with scalar bit tricks (~60 SALU instructions per group
// on the CU's one scalar unit).  Row i = word i >> 6, bit i & 63; bits past the last row are 0.
// One chunk per wave and step, 4 loads per operand in flight per lane: two chunks a grid stride apart (8 loads in flight)
// measured the same, 1.34 - 1.41 ms per 8 GB.
template <typename T, int CMP, int IEEE>
__global__ void __launch_bounds__(256) k_cmp(Ld<T> a, Ld<T> b, u64 *out, i64 n) {
    const int lane = threadIdx.x & 63;
    const i64 cstride = (i64)gridDim.x * (blockDim.x >> 6);
    const i64 nchunks = (n + 511) >> 9, nfull = n >> 9;
    const i64 nw = (n + 63) >> 6;
    const int src0 = (lane >> 1) << 2, src1 = (32 + (lane >> 1)) << 2;
    for (i64 c = (i64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < nchunks; c += cstride) {
        int pair[4];
        if (c < nfull) {
            Pair<T> x[4], y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                x[j] = ld2(a, (c * 4 + j) * 64 + lane);
                y[j] = ld2(b, (c * 4 + j) * 64 + lane);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                pair[j] = (CmpOp<T, CMP, IEEE>::apply(x[j].x, y[j].x) ? 1 : 0) | (CmpOp<T, CMP, IEEE>::apply(x[j].y, y[j].y) ? 2 : 0);
        } else {   // near the ragged end: row by row
            // (written with explicit flags: `if (r < n && apply(..)) pair |= 1` came out of hipcc 7.2 with a scalar-mask
            //  sequence that lost the Double.compare tie-break of the even rows -- caught by the special-values parity test)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const i64 r = (c * 4 + j) * 128 + 2 * lane;
                bool r0 = false, r1 = false;
                if (r < n) r0 = CmpOp<T, CMP, IEEE>::apply(a[r], b[r]);
                if (r + 1 < n) r1 = CmpOp<T, CMP, IEEE>::apply(a[r + 1], b[r + 1]);
                pair[j] = (r0 ? 1 : 0) | (r1 ? 2 : 0);
            }
        }
        u64 mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p0 = __builtin_amdgcn_ds_bpermute(src0, pair[j]);
            const int p1 = __builtin_amdgcn_ds_bpermute(src1, pair[j]);
            const u64 w0 = __ballot((p0 >> (lane & 1)) & 1);
            const u64 w1 = __ballot((p1 >> (lane & 1)) & 1);
            if (lane == 2 * j) mine = w0;
            if (lane == 2 * j + 1) mine = w1;
        }
        if (lane < 8 && c * 8 + lane < nw) out[c * 8 + lane] = mine;
    }
}

// Variant without cross-lane traffic: lane l takes rows l and l + 64 of every 128-row group (two loads of one element each
// instead of one load of two), so the two ballots ARE the group's two bitmap words -- no ds_bpermute, no per-lane shifts.
template <typename T, int CMP, int IEEE>
__global__ void __launch_bounds__(256) k_cmp_rows(Ld<T> a, Ld<T> b, u64 *out, i64 n) {
    const int lane = threadIdx.x & 63;
    const i64 cstride = (i64)gridDim.x * (blockDim.x >> 6);
    const i64 nchunks = (n + 511) >> 9, nfull = n >> 9;
    const i64 nw = (n + 63) >> 6;
    for (i64 c = (i64)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < nchunks; c += cstride) {
        bool r0[4], r1[4];
        if (c < nfull) {
            T x0[4], x1[4], y0[4], y1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const i64 r = (c * 4 + j) * 128 + lane;
                x0[j] = a[r]; x1[j] = a[r + 64];
                y0[j] = b[r]; y1[j] = b[r + 64];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                r0[j] = CmpOp<T, CMP, IEEE>::apply(x0[j], y0[j]);
                r1[j] = CmpOp<T, CMP, IEEE>::apply(x1[j], y1[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const i64 r = (c * 4 + j) * 128 + lane;
                bool t0 = false, t1 = false;
                if (r < n) t0 = CmpOp<T, CMP, IEEE>::apply(a[r], b[r]);
                if (r + 64 < n) t1 = CmpOp<T, CMP, IEEE>::apply(a[r + 64], b[r + 64]);
                r0[j] = t0; r1[j] = t1;
            }
        }
        u64 mine = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u64 w0 = __ballot(r0[j]), w1 = __ballot(r1[j]);
            if (lane == 2 * j) mine = w0;
            if (lane == 2 * j + 1) mine = w1;
        }
        if (lane < 8 && c * 8 + lane < nw) out[c * 8 + lane] = mine;
    }
}

static int cmp_grid(int64_t n) {
    static const int wgs_per_cu = getenv("QE_PN_CMP_WGS") ? atoi(getenv("QE_PN_CMP_WGS")) : 4;   // 16 waves per CU: 1.25 - 1.28 ms per 8 GB column; 32 waves 1.43 ms
    return grid_for((n + 511) / 512, 4, 256 * wgs_per_cu);   // 4 waves per workgroup, one 512-row chunk per wave and step
}
template <typename T, int IEEE> static void cmp_t(hipStream_t s, int cmp, const Opnd &a, const Opnd &b, u64 *out, int64_t n) {
    const int g = cmp_grid(n);
    // 4-byte columns (INT32, dictionary codes) take the row-per-lane form: k_cmp is bound by its per-group work, not by bytes
    // (~800 G rows/s for 8- and 4-byte columns alike), and without the cross-lane merge an int column runs 0.77 -> 0.43 ms per
    // 600 M rows; for 8-byte columns the two 8-byte loads cost more than the merge saves (1.51 against 1.22 ms per 1 B rows)
    with_const<C_NE + 1>(cmp, [&](auto c) {
        constexpr int CMP = decltype(c)::value;
        if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((k_cmp_rows<T, CMP, IEEE>), dim3(g), dim3(256), 0, s, mk<T>(a), mk<T>(b), out, (i64)n);
        else hipLaunchKernelGGL((k_cmp<T, CMP, IEEE>), dim3(g), dim3(256), 0, s, mk<T>(a), mk<T>(b), out, (i64)n);
    });
}
void compare(hipStream_t s, int type, int cmp, int ieee, Opnd a, Opnd b, uint64_t *out, int64_t n) {
    if (n <= 0) return;
    if (type == QE_DOUBLE && ieee) return cmp_t<double, 1>(s, cmp, a, b, (u64 *)out, n);   // the semantics differ on DOUBLE only
    with_type(type, [&](auto t) { cmp_t<QE_TAG_TYPE(t), 0>(s, cmp, a, b, (u64 *)out, n); });
}

template <typename T> struct NonzeroFn {
    Ld<T> b;
    __device__ bool operator()(i64 i) const { return b[i] != 0; }
};
void nonzero(hipStream_t s, int type, Opnd b, uint64_t *out, int64_t n) {
    with_type(type, [&](auto t) {
        typedef QE_TAG_TYPE(t) T;
        if constexpr (std::is_integral<T>::value) ballot(s, n, out, NonzeroFn<T>{mk<T>(b)});   // (a DOUBLE divisor is never asked)
    });
}

// ---- word-parallel logic (64 rows per word) ------------------------------------------------------------
struct WordOpFn {
    int op;
    const u64 *a, *b;
    u64 *out;
    __device__ void operator()(i64 i) const {
        const u64 x = a[i], y = b[i];
        u64 r;
        switch (op) {
        case W_AND: r = x & y; break;
        case W_OR: r = x | y; break;
        case W_XOR: r = x ^ y; break;
        case W_ANDNOT: r = x & ~y; break;
        case W_ORNOT: r = x | ~y; break;
        case W_XNOR: r = ~(x ^ y); break;
        case W_NOTAND: r = ~x & y; break;
        default: r = ~x | y; break;
        }
        out[i] = r;
    }
};
void word_op(hipStream_t s, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, int64_t nw) {
    map(s, nw, WordOpFn{op, (const u64 *)a, (const u64 *)b, (u64 *)out});
}
struct WordNotFn {
    const u64 *a;
    u64 *out;
    __device__ void operator()(i64 i) const { out[i] = ~a[i]; }
};
void word_not(hipStream_t s, const uint64_t *a, uint64_t *out, int64_t nw) { map(s, nw, WordNotFn{(const u64 *)a, (u64 *)out}); }
void word_fill(hipStream_t s, uint64_t v, uint64_t *out, int64_t nw) { map(s, nw, FillFn<i64>{(i64)v, (i64 *)out}); }

// Kleene three-valued AND / OR (Interpreter.kt:54-91; SURVEY 2.1 word-parallel form)
struct KleeneFn {
    int is_and;
    const u64 *va, *ka, *vb, *kb;
    u64 *vout, *kout;
    __device__ void operator()(i64 i) const {
        const u64 xa = ka ? ka[i] : ~0ull, xb = kb ? kb[i] : ~0ull;
        const u64 a = va[i] & xa, b = vb[i] & xb;   // value bits under a null are 0
        u64 v, k;
        if (is_and) {
            v = a & b;
            k = (xa & xb) | (xa & ~a) | (xb & ~b);   // false dominates null
        } else {
            v = a | b;
            k = (xa & xb) | a | b;                   // true dominates null
        }
        vout[i] = v;
        if (kout) kout[i] = k;
    }
};
void kleene(hipStream_t s, bool is_and, const uint64_t *va, const uint64_t *ka, const uint64_t *vb, const uint64_t *kb,
            uint64_t *vout, uint64_t *kout, int64_t nw) {
    map(s, nw, KleeneFn{is_and ? 1 : 0, (const u64 *)va, (const u64 *)ka, (const u64 *)vb, (const u64 *)kb, (u64 *)vout, (u64 *)kout});
}

// ---- IF -----------------------------------------------------------------------------------------------------
template <typename T> struct SelectFn {
    const u64 *cond;
    Ld<T> t, e;
    T *out;
    __device__ void operator()(i64 i) const {
        const bool c = (cond[i >> 6] >> (i & 63)) & 1ull;
        out[i] = c ? t[i] : e[i];
    }
};
void select(hipStream_t s, int type, const uint64_t *cond, Opnd t, Opnd e, void *out, int64_t n) {
    with_type(type, [&](auto tag) {
        typedef QE_TAG_TYPE(tag) T;
        map(s, n, SelectFn<T>{(const u64 *)cond, mk<T>(t), mk<T>(e), (T *)out});
    });
}
struct SelectWordsFn {
    const u64 *c, *t, *e;
    u64 *out;
    __device__ void operator()(i64 i) const { out[i] = (c[i] & t[i]) | (~c[i] & e[i]); }
};
void select_words(hipStream_t s, const uint64_t *c, const uint64_t *t, const uint64_t *e, uint64_t *out, int64_t nw) {
    map(s, nw, SelectWordsFn{(const u64 *)c, (const u64 *)t, (const u64 *)e, (u64 *)out});
}

// Gather of up to 8 value columns at the kept row ids, one output row per lane and step, 4 rows in flight per lane: every
// lane of every load carries a row (a masked one-row-per-lane compaction straight from the bitmap was measured 2.8x
// slower at 5 % selectivity: the address unit spends its cycles per wave instruction, not per active lane).
// Round 2, second try at 10 %: streaming the column and compacting through the keep bitmap (masked stores, or an LDS buffer per
// 512-row chunk and one coalesced store) took 1.71 - 1.78 ms per 8 GB column against 1.35 ms for this gather.
__global__ void __launch_bounds__(256) k_gather_multi(const GatherArgs a) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    i64 j = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    for (; j + 3 * stride < a.m; j += 4 * stride) {
        u32 r[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = __builtin_nontemporal_load(a.idx + j + q * stride);
        for (int c = 0; c < a.ncols; ++c) {
            if (a.width[c] == 8) {
                u64 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = ((const u64 *)a.src[c])[r[q]];
#pragma unroll
                for (int q = 0; q < 4; ++q) ((u64 *)a.dst[c])[j + q * stride] = v[q];
            } else {
                u32 v[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = ((const u32 *)a.src[c])[r[q]];
#pragma unroll
                for (int q = 0; q < 4; ++q) ((u32 *)a.dst[c])[j + q * stride] = v[q];
            }
        }
    }
    for (; j < a.m; j += stride) {
        const u32 r = a.idx[j];
        for (int c = 0; c < a.ncols; ++c) {
            if (a.width[c] == 8) ((u64 *)a.dst[c])[j] = ((const u64 *)a.src[c])[r];
            else ((u32 *)a.dst[c])[j] = ((const u32 *)a.src[c])[r];
        }
    }
}
void gather_multi(hipStream_t s, const GatherArgs &a) {
    if (a.m <= 0 || a.ncols <= 0) return;
    hipLaunchKernelGGL(k_gather_multi, dim3(grid_for((a.m + 3) / 4, 256, 256 * 8)), dim3(256), 0, s, a);
}

struct LookupCodesFn {
    const int *table;
    int ntable;
    const int *codes;
    int *out;
    __device__ void operator()(i64 j) const {
        const int c = codes[j];
        out[j] = (unsigned)c < (unsigned)ntable ? table[c] : -1;
    }
};
void lookup_codes(hipStream_t s, const int32_t *table, int32_t ntable, const int32_t *codes, int32_t *out, int64_t n) {
    map(s, n, LookupCodesFn{(const int *)table, (int)ntable, (const int *)codes, (int *)out});
}

// ---- set membership (IN / LIKE) ---------------------------------------------------------------------------------------
// The tables are read with ordinary cached loads: a table is small and every wave reads it, it stays in L2 beside the stream.
template <typename T> struct MemberBitsFn {
    const T *v;
    i64 base;
    u64 nbits;
    const u32 *table;
    __device__ bool operator()(i64 i) const {
        const u64 idx = (u64)(i64)v[i] - (u64)base;   // the garbage under a NULL lands outside [0, nbits) or on a bit nobody keeps
        return idx < nbits && ((table[idx >> 5] >> (u32)(idx & 31ull)) & 1u) != 0u;
    }
};
void member_bits(hipStream_t s, int type, const void *values, long long base, long long nbits, const uint32_t *table, uint64_t *out, int64_t n) {
    with_type(type, [&](auto t) {
        typedef QE_TAG_TYPE(t) T;
        if constexpr (std::is_integral<T>::value)   // (integers and dictionary codes only: a DOUBLE value goes through the hash set)
            ballot(s, n, out, MemberBitsFn<T>{(const T *)values, (i64)base, (u64)nbits, (const u32 *)table});
    });
}

template <typename T> __device__ __forceinline__ u64 member_image(T v) { return (u64)(i64)v; }
template <> __device__ __forceinline__ u64 member_image<double>(double v) {
    return v != v ? 0x7ff8000000000000ull : __builtin_bit_cast(u64, v);   // Double.doubleToLongBits
}
template <typename T> struct MemberHashFn {   // the kernel's arguments
    const T *v;
    const u64 *table;
};
template <typename T> struct MemberHashTest {   // and its row test: the table's header (wave-uniform) in registers
    const T *v;
    const u64 *table;
    u64 mask, home_mask, empty;
    u32 probe;
    __device__ bool operator()(i64 i) const {
        const u64 image = member_image<T>(v[i]);
        const u64 home = (u64)(u32)((image * 0x9E3779B97F4A7C15ull) >> 32) & home_mask;
        bool r = false;
        for (u32 j = 0; j < probe; ++j) r |= table[4 + ((home + j) & mask)] == image;   // independent loads: every address is known up front
        return r && image != empty;
    }
};
template <typename T> __device__ __forceinline__ MemberHashTest<T> row_test(const MemberHashFn<T> &f) {
    const u64 h0 = f.table[0], home_mask = f.table[1], empty = f.table[2];
    return MemberHashTest<T>{f.v, f.table, h0 & 0xffffffffull, home_mask, empty, (u32)(h0 >> 32)};
}
void member_hash(hipStream_t s, int type, const void *values, const uint64_t *table, uint64_t *out, int64_t n) {
    with_type(type, [&](auto t) {
        typedef QE_TAG_TYPE(t) T;
        ballot(s, n, out, MemberHashFn<T>{(const T *)values, (const u64 *)table});
    });
}

}  // namespace pn
}  // namespace qe
