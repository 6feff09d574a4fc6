// qe_window.hip -- window functions over a sorted result (host side: qe_window.cpp).
//
// The rows arrive sorted by (partition columns, order keys).  One kernel marks where a partition and where a group of peers
// starts, as two bitmaps (a u64 word per wave from __ballot).  Everything else is a SEGMENTED INCLUSIVE SCAN over the rows
// that restarts at every partition start, always in the same three steps of a fixed shape:
//   reduce     one workgroup per tile of T = 2048 rows: wave w scans rows [512 w, 512 w + 512) of the tile as 8 words of 64
//              rows (a segmented __shfl_up scan under the word's start bits, the running value carried from word to word),
//              the four wave aggregates are folded in wave order -> {aggregate since the tile's last start, tile has a start}
//   tile scan  ONE workgroup of 1024 lanes scans the tile aggregates, 1024 per trip, the carry going from trip to trip
//              -> what every tile inherits from the rows before it
//   downsweep  the reduce again, now seeded with the tile's carry, and the rows' results are written
// Which values are combined with which is a function of the row count and the start bits alone: no atomics, no look-back,
// so a running f64 SUM has the same bits on every run and every context.
//
// FRAMES (ROWS BETWEEN p PRECEDING AND f FOLLOWING).  The same triple also runs in REVERSE (from row n - 1 down; a segment
// ends where the next row starts a partition, and at row n - 1) and with EXTRA BREAKS at every multiple of a block width W
// that are made on the fly (a __ballot per word, no bitmap).  With W = p + f + 1 the forward scan P restarts at partition and
// block starts, the reverse scan S at partition and block ends, and a frame [lo, hi] -- at most W rows, so it touches at most
// two adjacent blocks -- is P[hi], S[lo] or combine(S[lo], P[hi]) (win_frame_kernel).  Only rows inside the frame are ever
// combined: no difference of prefixes, so a value that has left the frame leaves no trace.
// A reverse scan is the forward one over the MIRRORED rows: logical row q is physical row npad - 1 - q, npad = tiles * T.  A
// word of 64 logical rows is one physical word with its lanes reversed, so bitmap words are read and written through
// __brevll and everything between the loads and the stores is the forward code.
#include <hip/hip_runtime.h>

#include "qe_kernels.h"
#include "qe_sort_image.h"

namespace qe {

// ---- boundary flags ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) win_flags_kernel(const WinFlagArgs a) {
    const i64 padded = (a.n + 63) & ~63ll;   // whole waves: every lane takes part in the shuffles and ballots
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    u64 starts = 0;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < padded; j += stride) {
        const bool in = j < a.n;
        const i64 row = !in ? 0 : a.perm ? (i64)a.perm[j] : j;
        const i64 prev_row = (!in || j == 0) ? 0 : a.perm ? (i64)a.perm[j - 1] : j - 1;   // read by lane 0 only
        bool pdiff = in && j == 0, odiff = false;
        for (int k = 0; k < a.nkeys; ++k) {
            u64 img = 0;
            int valid = 0;
            if (in) {
                valid = (!a.validity[k] || bit_at(a.validity[k], row)) ? 1 : 0;
                img = sort_image(a.type[k], a.data[k], a.validity[k], a.ranks[k], a.nranks[k], row);
            }
            u64 pimg = __shfl_up(img, 1, 64);
            int pvalid = __shfl_up(valid, 1, 64);
            if (lane == 0 && in && j > 0) {   // the row before this wave's first
                pvalid = (!a.validity[k] || bit_at(a.validity[k], prev_row)) ? 1 : 0;
                pimg = sort_image(a.type[k], a.data[k], a.validity[k], a.ranks[k], a.nranks[k], prev_row);
            }
            const bool d = in && j > 0 && (img != pimg || valid != pvalid);
            if (k < a.npart) pdiff = pdiff || d;
            else odiff = odiff || d;
        }
        const u64 pw = __ballot(pdiff), ow = __ballot(pdiff || odiff);
        if (lane == 0) {
            a.pstart[j >> 6] = pw;
            a.peer[j >> 6] = ow;
            starts += (u64)__popcll(pw);
        }
    }
    if (lane == 0 && starts) atomicAdd(a.npartitions, starts);   // an integer count: the order of arrival does not show
}
void launch_win_flags(hipStream_t s, const WinFlagArgs &a) {
    if (a.n <= 0) return;
    const i64 blocks = (a.n + 255) / 256;
    hipLaunchKernelGGL(win_flags_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, a);
}

// ---- the scanned value ---------------------------------------------------------------------------------------------------
// {v, c}: SUM: sum of the valid values and their count; MIN / MAX: the extreme (meaningless while c == 0) and the count;
// INDEX: c = greatest row index whose bit is set (0: none, or row 0 -- whose bit is always set where it is asked for)
struct Item {
    double v;
    u32 c;
};

// MIN / MAX of two values as qe_filter_groupby decided them: NaN wins, -0.0 below +0.0
__device__ __forceinline__ double win_min(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    if (a < b) return a;
    if (b < a) return b;
    return __builtin_bit_cast(double, __builtin_bit_cast(u64, a) | __builtin_bit_cast(u64, b));   // equal: -0.0 if either is
}
__device__ __forceinline__ double win_max(double a, double b) {
    if (a != a) return a;
    if (b != b) return b;
    if (a < b) return b;
    if (b < a) return a;
    return __builtin_bit_cast(double, __builtin_bit_cast(u64, a) & __builtin_bit_cast(u64, b));   // equal: +0.0 if either is
}

template <int OP> __device__ __forceinline__ Item identity() { return Item{0.0, 0u}; }

// a: the earlier rows, b: the later ones
template <int OP> __device__ __forceinline__ Item combine(const Item a, const Item b) {
    Item r;
    if (OP == QE_WSCAN_SUM) {
        r.v = a.v + b.v;
        r.c = a.c + b.c;
    } else if (OP == QE_WSCAN_INDEX) {
        r.v = 0.0;
        r.c = a.c > b.c ? a.c : b.c;
    } else {
        r.c = a.c + b.c;
        if (a.c == 0) r.v = b.v;
        else if (b.c == 0) r.v = a.v;
        else r.v = OP == QE_WSCAN_MIN ? win_min(a.v, b.v) : win_max(a.v, b.v);
    }
    return r;
}

// Segmented inclusive scan of one value per lane under the wave's start bits: lane l gets the combination of the lanes from
// the nearest start at or below l (lane 0 when there is none) up to l.
template <int OP> __device__ __forceinline__ Item wave_seg_scan(Item x, u64 starts, int lane) {
    const u64 below = starts & (~0ull >> (63 - lane));
    const int first = below ? 63 - __clzll((long long)below) : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        Item t;
        t.v = __shfl_up(x.v, d, 64);
        t.c = __shfl_up(x.c, d, 64);
        if (lane - d >= first) x = combine<OP>(t, x);
    }
    return x;
}

// j: the physical row of this lane, q: its place in scan order (== j in a forward scan); bit `lane` of valid_word is its bit
template <int OP> __device__ __forceinline__ Item load_item(const WinScanArgs &a, i64 j, i64 q, u64 valid_word, int lane) {
    Item x = identity<OP>();
    const bool set = j < a.n && ((valid_word >> lane) & 1ull);
    if (OP == QE_WSCAN_INDEX) {
        x.c = set ? (u32)q : 0u;
        return x;
    }
    if (!set) return x;
    x.c = 1u;
    if (a.data) {   // converted as the GROUP BY aggregates convert their input: (double)
        switch (a.type) {
        case QE_DOUBLE: x.v = ((const double *)a.data)[j]; break;
        case QE_INT64: x.v = (double)((const i64 *)a.data)[j]; break;
        default: x.v = (double)((const int *)a.data)[j]; break;
        }
    }
    return x;
}

constexpr int kWinWaveWords = kWinTileRows / 64 / 4;   // words of 64 rows one wave scans: 8

// Where the 64 rows of one word live.  base: the word's first row in scan order.
template <bool REV> __device__ __forceinline__ i64 word_rows(const WinScanArgs &a, i64 base) {
    return REV ? a.ntiles * kWinTileRows - 64 - base : base;   // first PHYSICAL row of the word
}
template <bool REV> __device__ __forceinline__ i64 lane_row(i64 pbase, int lane) { return REV ? pbase + 63 - lane : pbase + lane; }

// The word of `bits` (a partition-start bitmap; null: no bit) for the physical rows [pbase, pbase + 64), lane order of the scan.
// Forward: the bits themselves.  Reverse: bit of row j = row j ENDS a partition (row j + 1 starts one, or j == n - 1).
template <bool REV> __device__ __forceinline__ u64 edge_word(const u64 *bits, i64 pbase, i64 n) {
    if (!REV) return bits ? bits[pbase >> 6] : 0ull;
    u64 e = 0ull;
    if (bits) {
        e = bits[pbase >> 6] >> 1;
        if (pbase + 64 < n) e |= bits[(pbase >> 6) + 1] << 63;
    }
    if (((n - 1) >> 6) == (pbase >> 6)) e |= 1ull << ((n - 1) & 63);
    return __brevll(e);
}

// The tile's rows scanned RELATIVE to the start of each wave's 512 rows: loc[w] = result of this lane's row in word w of its
// wave, counting from the wave's first row or the nearest start; bit w of `seen` = a start stands between the wave's first
// row and this row (inclusive), so nothing from before the wave reaches it.  wave_total / wave_started: the wave's aggregate.
// wave_base and every "before" are in scan order; a.block > 0 adds a start at every block edge (every lane of the wave is
// here: the __ballot is whole).
template <int OP, bool REV>
__device__ __forceinline__ void wave_local_scan(const WinScanArgs &a, i64 wave_base, int lane, Item (&loc)[kWinWaveWords], u32 &seen,
                                                Item &wave_total, bool &wave_started) {
    Item run = identity<OP>();
    bool started = false;   // wave-uniform
    seen = 0;
#pragma unroll
    for (int w = 0; w < kWinWaveWords; ++w) {
        const i64 base = wave_base + (i64)w * 64;
        const i64 pbase = word_rows<REV>(a, base);
        const bool word_in = pbase < a.n;   // wave-uniform
        const i64 j = lane_row<REV>(pbase, lane);
        u64 starts = word_in ? edge_word<REV>(a.pstart, pbase, a.n) : 0ull;
        if (a.block > 0) {   // wave-uniform; j < n < 2^32 and block < 2^32
            const u32 r = j < a.n ? (u32)j % (u32)a.block : 1u;
            starts |= __ballot(j < a.n && r == (REV ? (u32)a.block - 1u : 0u));
        }
        u64 valid_word;
        if (!word_in) valid_word = 0ull;
        else if (REV && OP == QE_WSCAN_INDEX) valid_word = edge_word<REV>(a.validity, pbase, a.n);
        else valid_word = !a.validity ? ~0ull : REV ? __brevll(a.validity[pbase >> 6]) : a.validity[pbase >> 6];
        Item x = load_item<OP>(a, j, base + lane, valid_word, lane);
        x = wave_seg_scan<OP>(x, starts, lane);
        const bool below = (starts & (~0ull >> (63 - lane))) != 0ull;
        if (!below) x = combine<OP>(run, x);
        loc[w] = x;
        if (started || below) seen |= 1u << w;
        run.v = __shfl(x.v, 63, 64);
        run.c = __shfl(x.c, 63, 64);
        started = started || starts != 0ull;
    }
    wave_total = run;
    wave_started = started;
}

// One row's result through the output modes; returns whether the row has a value (its validity bit).
__device__ __forceinline__ bool store_item(int out_mode, void *out, u32 *out_c, i64 j, bool in, const Item x) {
    const bool have = in && x.c != 0u;
    switch (out_mode) {
    case QE_WOUT_SUM:      // + 0.0: the accumulator starts from 0.0 (Accumulators.kt:40), so a prefix of only -0.0 gives +0.0
        if (in) ((double *)out)[j] = have ? x.v + 0.0 : 0.0;
        break;
    case QE_WOUT_MINMAX:
        if (in) ((double *)out)[j] = have ? x.v : 0.0;
        break;
    case QE_WOUT_AVG:
        if (in) ((double *)out)[j] = have ? (x.v + 0.0) / (double)x.c : 0.0;
        break;
    case QE_WOUT_COUNT:
        if (in) ((double *)out)[j] = (double)x.c;
        break;
    case QE_WOUT_COUNT_I64:
        if (in) ((i64 *)out)[j] = (i64)x.c;
        break;
    case QE_WOUT_ITEM:     // the scanned pair itself, for win_frame_kernel
        if (in) {
            ((double *)out)[j] = x.v;
            out_c[j] = x.c;
        }
        break;
    default:
        if (in) ((u32 *)out)[j] = x.c;
        break;
    }
    return have;
}

// ---- step 1: tile aggregates -------------------------------------------------------------------------------------------
template <int OP, bool REV> __global__ void __launch_bounds__(256) win_reduce_kernel(const WinScanArgs a) {
    __shared__ double s_v[4];
    __shared__ u32 s_c[4], s_f[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Item loc[kWinWaveWords];
    u32 seen;
    Item total;
    bool started;
    wave_local_scan<OP, REV>(a, (i64)blockIdx.x * kWinTileRows + (i64)wave * (kWinTileRows / 4), lane, loc, seen, total, started);
    if (lane == 0) {
        s_v[wave] = total.v;
        s_c[wave] = total.c;
        s_f[wave] = started ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Item agg = identity<OP>();
        u32 f = 0;
        for (int w = 0; w < 4; ++w) {
            const Item t{s_v[w], s_c[w]};
            agg = s_f[w] ? t : combine<OP>(agg, t);
            f |= s_f[w];
        }
        a.tile_v[blockIdx.x] = agg.v;
        a.tile_c[blockIdx.x] = agg.c;
        a.tile_f[blockIdx.x] = f;
    }
}

// ---- step 2: one workgroup over the tile aggregates, kWinTripTiles per trip ------------------------------------------------
// (tiles in scan order: the kernel is the same for both directions)
// carry[i] = combination of the tiles before tile i back to the last tile that holds a start (that tile's aggregate already
// counts from its last start only); the identity for tile 0
template <int OP> __global__ void __launch_bounds__(kWinTripTiles) win_tile_scan_kernel(const WinScanArgs a) {
    __shared__ double s_v[kWinTripTiles / 64];
    __shared__ u32 s_c[kWinTripTiles / 64], s_f[kWinTripTiles / 64];
    __shared__ double s_carry_v;
    __shared__ u32 s_carry_c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        s_carry_v = 0.0;
        s_carry_c = 0u;
        a.carry_v[0] = 0.0;
        a.carry_c[0] = 0u;
    }
    __syncthreads();
    for (i64 b = 0; b < a.ntiles; b += kWinTripTiles) {
        const i64 i = b + threadIdx.x;
        const bool in = i < a.ntiles;
        Item x = identity<OP>();
        u32 f = 0;
        if (in) {
            x.v = a.tile_v[i];
            x.c = a.tile_c[i];
            f = a.tile_f[i];
        }
        const u64 starts = __ballot(f != 0u);
        x = wave_seg_scan<OP>(x, starts, lane);
        const bool below = (starts & (~0ull >> (63 - lane))) != 0ull;
        if (lane == 63) {
            s_v[wave] = x.v;
            s_c[wave] = x.c;
            s_f[wave] = starts != 0ull ? 1u : 0u;
        }
        __syncthreads();
        Item p{s_carry_v, s_carry_c};
        for (int w = 0; w < wave; ++w) {
            const Item t{s_v[w], s_c[w]};
            p = s_f[w] ? t : combine<OP>(p, t);
        }
        const Item incl = below ? x : combine<OP>(p, x);
        if (in && i + 1 < a.ntiles) {   // what tile i + 1 inherits
            a.carry_v[i + 1] = incl.v;
            a.carry_c[i + 1] = incl.c;
        }
        __syncthreads();   // every lane has read the carry and the wave aggregates of this trip
        if (threadIdx.x == kWinTripTiles - 1) {
            s_carry_v = incl.v;
            s_carry_c = incl.c;
        }
        __syncthreads();
    }
}

// ---- step 3: downsweep ---------------------------------------------------------------------------------------------------
template <int OP, bool REV> __global__ void __launch_bounds__(256) win_downsweep_kernel(const WinScanArgs a) {
    __shared__ double s_v[4];
    __shared__ u32 s_c[4], s_f[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 wave_base = (i64)blockIdx.x * kWinTileRows + (i64)wave * (kWinTileRows / 4);
    Item loc[kWinWaveWords];
    u32 seen;
    Item total;
    bool started;
    wave_local_scan<OP, REV>(a, wave_base, lane, loc, seen, total, started);
    if (lane == 0) {
        s_v[wave] = total.v;
        s_c[wave] = total.c;
        s_f[wave] = started ? 1u : 0u;
    }
    __syncthreads();
    Item p{a.carry_v[blockIdx.x], a.carry_c[blockIdx.x]};   // what reaches this wave's first row from before it
    for (int w = 0; w < wave; ++w) {
        const Item t{s_v[w], s_c[w]};
        p = s_f[w] ? t : combine<OP>(p, t);
    }
#pragma unroll
    for (int w = 0; w < kWinWaveWords; ++w) {
        const i64 pbase = word_rows<REV>(a, wave_base + (i64)w * 64);
        if (pbase >= a.n) continue;   // wave-uniform
        const i64 j = lane_row<REV>(pbase, lane);
        Item x = ((seen >> w) & 1u) ? loc[w] : combine<OP>(p, loc[w]);
        if (REV && OP == QE_WSCAN_INDEX) x.c = (u32)(a.ntiles * kWinTileRows - 1 - (i64)x.c);   // place in scan order -> row
        const bool have = store_item(a.out_mode, a.out, a.out_c, j, j < a.n, x);
        if (a.out_valid) {   // wave-uniform
            const u64 word = __ballot(have);
            if (lane == 0) a.out_valid[pbase >> 6] = REV ? __brevll(word) : word;
        }
    }
}

template <int OP, bool REV> static void win_scan_launch(hipStream_t s, const WinScanArgs &a) {
    hipLaunchKernelGGL((win_reduce_kernel<OP, REV>), dim3((unsigned)a.ntiles), dim3(256), 0, s, a);
    hipLaunchKernelGGL(win_tile_scan_kernel<OP>, dim3(1), dim3(kWinTripTiles), 0, s, a);
    hipLaunchKernelGGL((win_downsweep_kernel<OP, REV>), dim3((unsigned)a.ntiles), dim3(256), 0, s, a);
}
template <int OP> static void win_scan_direction(hipStream_t s, const WinScanArgs &a) {
    if (a.reverse) win_scan_launch<OP, true>(s, a);
    else win_scan_launch<OP, false>(s, a);
}
void launch_win_scan(hipStream_t s, const WinScanArgs &a) {
    if (a.n <= 0) return;
    switch (a.op) {
    case QE_WSCAN_SUM: win_scan_direction<QE_WSCAN_SUM>(s, a); break;
    case QE_WSCAN_MIN: win_scan_direction<QE_WSCAN_MIN>(s, a); break;
    case QE_WSCAN_MAX: win_scan_direction<QE_WSCAN_MAX>(s, a); break;
    default: win_scan_direction<QE_WSCAN_INDEX>(s, a); break;
    }
}

// ---- a framed aggregate out of the scanned pairs -------------------------------------------------------------------------------
template <int OP> __global__ void __launch_bounds__(256) win_frame_kernel(const WinFrameArgs a) {
    const i64 padded = (a.n + 63) & ~63ll;   // whole waves for the ballot
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < padded; j += stride) {
        const bool in = j < a.n;
        Item x = identity<OP>();
        if (in) {
            const i64 s = a.start[j], e = a.end[j];
            const i64 lo = a.preceding < 0 ? s : (j - a.preceding > s ? j - a.preceding : s);
            const i64 hi = a.following < 0 ? e : (j + a.following < e ? j + a.following : e);
            const Item fwd{a.p_v ? a.p_v[hi] : 0.0, a.p_v ? a.p_c[hi] : 0u}, rev{a.s_v ? a.s_v[lo] : 0.0, a.s_v ? a.s_c[lo] : 0u};
            if (a.preceding < 0) {
                x = fwd;                                  // the plain running scan at hi
            } else if (a.following < 0) {
                x = rev;                                  // the plain reverse-running scan at lo
            } else {                                      // P and S restart at the edges of blocks of W rows; lo, hi, W < 2^32
                const u32 W = (u32)(a.preceding + a.following + 1);
                const i64 bs = hi - (i64)((u32)hi % W), be = lo - (i64)((u32)lo % W) + (i64)W - 1;
                if ((bs > s ? bs : s) == lo) x = fwd;             // the frame begins where P last restarted
                else if ((be < e ? be : e) == hi) x = rev;        // the frame ends where S last restarted
                else x = combine<OP>(rev, fwd);                   // adjacent blocks: lo .. block end, block start .. hi
            }
        }
        const bool have = store_item(a.out_mode, a.out, nullptr, j, in, x);
        if (a.out_valid) {   // wave-uniform
            const u64 word = __ballot(have);
            if (lane == 0) a.out_valid[j >> 6] = word;
        }
    }
}
void launch_win_frame(hipStream_t s, const WinFrameArgs &a) {
    if (a.n <= 0) return;
    const i64 blocks = (a.n + 255) / 256;
    const dim3 g((unsigned)(blocks < 8192 ? blocks : 8192));
    switch (a.op) {
    case QE_WSCAN_SUM: hipLaunchKernelGGL(win_frame_kernel<QE_WSCAN_SUM>, g, dim3(256), 0, s, a); break;
    case QE_WSCAN_MIN: hipLaunchKernelGGL(win_frame_kernel<QE_WSCAN_MIN>, g, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL(win_frame_kernel<QE_WSCAN_MAX>, g, dim3(256), 0, s, a); break;
    }
}

// ---- ROW_NUMBER / RANK ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) win_rank_kernel(const u32 *start, const u32 *first, i64 n, i64 *out) {
    const i64 stride = (i64)gridDim.x * 256;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < n; j += stride) out[j] = (first ? (i64)first[j] : j) - (i64)start[j] + 1;
}
void launch_win_rank(hipStream_t s, const uint32_t *start, const uint32_t *first, int64_t n, int64_t *out) {
    if (n <= 0) return;
    const i64 blocks = (n + 255) / 256;
    hipLaunchKernelGGL(win_rank_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, start, first, (i64)n, (i64 *)out);
}

// ---- LAG / LEAD, FIRST_VALUE / LAST_VALUE ----------------------------------------------------------------------------------------
// A gather at j + delta.  end null: the row must exist in the same partition (LAG / LEAD); end given: the row is clamped into
// the partition [start[j], end[j]] (the frame's first or last row).  WIDTH 8 / 4: a value column; 0: a bitmap column (BOOLEAN)
template <int WIDTH>
__global__ void __launch_bounds__(256) win_shift_kernel(const void *src, const u64 *src_valid, const u32 *start, const u32 *end, i64 n, i64 delta,
                                                        void *out, u64 *out_valid) {
    const i64 padded = (n + 63) & ~63ll;
    const i64 stride = (i64)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < padded; j += stride) {
        i64 t = j + delta;
        bool ok;
        if (end) {
            ok = j < n;
            if (ok) {
                const i64 s0 = start[j], e0 = end[j];
                t = t < s0 ? s0 : t > e0 ? e0 : t;
            }
        } else {
            ok = j < n && t >= 0 && t < n && start[t] == start[j];   // the same partition: the same start index
        }
        if (WIDTH == 8) {
            if (j < n) ((u64 *)out)[j] = ok ? ((const u64 *)src)[t] : 0ull;
        } else if (WIDTH == 4) {
            if (j < n) ((u32 *)out)[j] = ok ? ((const u32 *)src)[t] : 0u;
        } else {
            const u64 word = __ballot(ok && bit_at((const u64 *)src, t));
            if (lane == 0) ((u64 *)out)[j >> 6] = word;
        }
        if (out_valid) {   // wave-uniform; null: the output column carries no validity (a clamped gather of a column without one)
            const u64 vword = __ballot(ok && (!src_valid || bit_at(src_valid, t)));
            if (lane == 0) out_valid[j >> 6] = vword;
        }
    }
}
void launch_win_shift(hipStream_t s, int width, const void *src, const uint64_t *src_valid, const uint32_t *start, const uint32_t *end, int64_t n,
                      int64_t delta, void *out, uint64_t *out_valid) {
    if (n <= 0) return;
    const i64 blocks = (n + 255) / 256;
    const dim3 g((unsigned)(blocks < 8192 ? blocks : 8192));
    if (width == 8)
        hipLaunchKernelGGL(win_shift_kernel<8>, g, dim3(256), 0, s, src, (const u64 *)src_valid, start, end, (i64)n, (i64)delta, out, (u64 *)out_valid);
    else if (width == 4)
        hipLaunchKernelGGL(win_shift_kernel<4>, g, dim3(256), 0, s, src, (const u64 *)src_valid, start, end, (i64)n, (i64)delta, out, (u64 *)out_valid);
    else
        hipLaunchKernelGGL(win_shift_kernel<0>, g, dim3(256), 0, s, src, (const u64 *)src_valid, start, end, (i64)n, (i64)delta, out, (u64 *)out_valid);
}

}  // namespace qe
