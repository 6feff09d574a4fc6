// qe_join.hip -- hash equi-join on the device: build once, probe results or batches.
//
// BUILD   one canonical u64 image per key column and row (the equality of DESIGN 4: every NaN one value, -0.0 != 0.0, a
//         STRING its canonical code in the build dictionary), mixed into a 64-bit hash; rows with a NULL key are marked.
//         The host sorts (hash, row) STABLY on the top hash bits (qe_sort.hip), moves the marked rows behind the others
//         and gathers the images into that order, so that a bucket of the directory over the top hash bits is one
//         contiguous run in which the entries of one sorted hash prefix -- hence all entries with equal keys -- stand in
//         build-row order (the sort covers whole 4-bit digits, so it may look at up to 3 hash bits below the bucket bits).
// PROBE   two passes with nothing but positions in between: (1) every probe row hashes its key, walks its bucket and
//         counts the entries whose EVERY image is equal; (2) after an exclusive 64-bit scan of the counts the same walk
//         writes (probe row, build row) pairs at the scanned offsets.  The order of the output is therefore the order of
//         a nested loop with the probe side outside, whatever the order in which the waves run; the only atomics are an
//         integer add (rows with a key), an integer max (longest bucket) and an integer OR (OUTER), all independent of
//         arrival order.
// OUTER   RIGHT / FULL: pass 1 also ORs the bit of every build row it finds equal into a bitmap over build rows that belongs
//         to the CALL (the table is read only); the bit is read first and the atomic skipped when it is set.  The final
//         bitmap is the OR of the same bits in whatever order they arrive.  Complemented, ranked and compacted
//         (qe_scan.h) it is the TAIL: the build rows nobody matched, ascending, appended to the pair lists with probe row
//         0xFFFFFFFF.  With a null bitmap (the other four types) pass 1 is the instantiation without the marks.
// GATHER  one launch of the shared gathers (qe_kernels.hip) per output column through the pair lists; row 0xFFFFFFFF
//         ("none": the build row under LEFT / FULL, the probe row of a tail row) gives a zeroed value and validity 0.
#include <hip/hip_runtime.h>

#include "qe_kernels.h"
#include "qe_scan.h"

namespace qe {

typedef unsigned long long u64;
typedef long long i64;
typedef unsigned int u32;

namespace {

constexpr u32 kNone = 0xFFFFFFFFu;

__device__ __forceinline__ bool jbit_at(const u64 *bm, i64 i) { return (bm[i >> 6] >> (i & 63)) & 1ull; }

// splitmix64 finaliser: every input bit reaches the top bits the directory is indexed with
__device__ __forceinline__ u64 mix64(u64 x) {
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// The images of row i's key; false when the key matches nothing: a NULL in any key column, or a STRING the build
// dictionary does not hold (or the garbage code under a NULL of a column that lost its bitmap).
__device__ __forceinline__ bool key_images(const JoinKeyCols &kc, i64 i, u64 img[4]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        img[k] = 0;
        if (k >= kc.nkeys) continue;
        if (kc.validity[k] && !jbit_at(kc.validity[k], i)) {
            ok = false;
            continue;
        }
        switch (kc.type[k]) {
        case QE_DOUBLE: {   // Double.equals: the bits, every NaN the canonical one
            const double d = ((const double *)kc.data[k])[i];
            img[k] = d != d ? 0x7ff8000000000000ull : __builtin_bit_cast(u64, d);
            break;
        }
        case QE_INT64: img[k] = (u64)((const i64 *)kc.data[k])[i]; break;
        case QE_INT32: img[k] = (u64)(i64)((const int *)kc.data[k])[i]; break;
        case QE_STRING: {
            int c = ((const int *)kc.data[k])[i];
            if ((u32)c >= (u32)kc.ncodes[k]) {
                ok = false;
                break;
            }
            if (kc.remap[k]) c = kc.remap[k][c];
            if (c < 0) ok = false;
            img[k] = (u64)(u32)c;
            break;
        }
        default: img[k] = jbit_at((const u64 *)kc.data[k], i) ? 1ull : 0ull; break;   // BOOLEAN bitmap
        }
    }
    return ok;
}

__device__ __forceinline__ u64 key_hash(const u64 img[4], int nkeys, u64 mask) {
    u64 h = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < nkeys) h = mix64(h + 0x9e3779b97f4a7c15ull + img[k]);
    return h & mask;
}

// ---- build ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) join_build_keys_kernel(const JoinBuildArgs a) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const i64 padded = (a.n + 63) & ~63ll;   // whole waves: every lane takes part in the ballot
    u32 nvalid = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < padded; i += stride) {
        bool ok = false;
        if (i < a.n) {
            u64 img[4];
            ok = key_images(a.kc, i, img);
            a.hash[i] = key_hash(img, a.kc.nkeys, a.mask);
            a.rows[i] = (u32)i;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < a.kc.nkeys) a.img[k][i] = img[k];
        }
        const u64 m = __ballot(ok);
        if ((threadIdx.x & 63) == 0) {
            a.valid_words[i >> 6] = m;
            nvalid += (u32)__popcll(m);
        }
    }
    if ((threadIdx.x & 63) == 0 && nvalid) atomicAdd(a.nvalid, (u64)nvalid);
}

// dir[b] = first sorted entry whose top `dbits` hash bits are >= b, for b = 0 .. 2^dbits (dir[2^dbits] = m)
__global__ void __launch_bounds__(256) join_directory_kernel(const u64 *shash, i64 m, int dbits, u32 *dir, i64 nentries) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 b = (i64)blockIdx.x * blockDim.x + threadIdx.x; b < nentries; b += stride) {
        i64 lo = 0, hi = m;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if ((i64)(shash[mid] >> (64 - dbits)) < b) lo = mid + 1;
            else hi = mid;
        }
        dir[b] = (u32)lo;
    }
}

// ---- probe ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool entry_equal(const JoinTableView &t, u32 s, const u64 img[4]) {
    bool eq = t.img[0][s] == img[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (k < t.nkeys) eq = eq && t.img[k][s] == img[k];
    return eq;
}

// pass 1: matches per probe row (LEFT: at least 1; SEMI / ANTI: 0 or 1), the sorted position of the first match, the sum of
// every block of 256 rows.  MARK (RIGHT / FULL, a.matched set): also the marks of the matched build rows; the other types run
// the instantiation without them, which is the kernel as it was
template <bool MARK> __global__ void __launch_bounds__(256) join_count_kernel(const JoinProbeArgs a) {
    __shared__ u64 s_sum[4];
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    u32 cnt = 0, first = kNone, walked = 0;
    if (i < a.n) {
        u64 img[4];
        if (key_images(a.kc, i, img)) {
            const u64 h = key_hash(img, a.kc.nkeys, a.t.mask);
            const u32 b = (u32)(h >> (64 - a.t.dbits));
            const u32 s0 = a.t.dir[b], s1 = a.t.dir[b + 1];
            const bool first_only = a.join_type == QE_JOIN_SEMI || a.join_type == QE_JOIN_ANTI;
            for (u32 s = s0; s < s1; ++s) {
                ++walked;
                if (entry_equal(a.t, s, img)) {   // a shared hash alone is never a match
                    if (MARK) {   // the build row has been matched.  Many probe rows hit one build row and 64 build rows share
                                  // a word: only a lane that still sees the bit clear goes to the atomic (a stale read costs
                                  // an OR that changes nothing)
                        const u32 r = a.t.rows[s];
                        const u64 bit = 1ull << (r & 63);
                        if (!(__atomic_load_n(a.matched + (r >> 6), __ATOMIC_RELAXED) & bit)) atomicOr(a.matched + (r >> 6), bit);
                    }
                    if (cnt == 0) first = s;
                    ++cnt;
                    if (first_only) break;
                }
            }
        }
        if (a.join_type == QE_JOIN_LEFT) cnt = cnt ? cnt : 1u;
        else if (a.join_type == QE_JOIN_SEMI) cnt = cnt ? 1u : 0u;
        else if (a.join_type == QE_JOIN_ANTI) cnt = cnt ? 0u : 1u;
        a.cnt[i] = cnt;
        if (a.first) a.first[i] = first;
    }
    u64 sum = cnt;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        const u32 o = __shfl_xor(walked, d, 64);
        walked = o > walked ? o : walked;
    }
    if ((threadIdx.x & 63) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        // one address for the whole grid: only a wave that raises the maximum it can see goes to the atomic (a stale read
        // costs an atomic that changes nothing; the final value is the maximum either way)
        if (walked > __atomic_load_n(a.longest, __ATOMIC_RELAXED)) atomicMax(a.longest, walked);
    }
    __syncthreads();
    if (threadIdx.x == 0) a.blocksum[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// pass 2: the pairs of probe row i at offset (block offset + the counts of the rows before it in its block)
__global__ void __launch_bounds__(256) join_write_kernel(const JoinProbeArgs a) {
    __shared__ u64 s_wave[4];
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const u32 cnt = i < a.n ? a.cnt[i] : 0u;
    u64 block_total;
    const u64 off = a.blocksum[blockIdx.x] + block_excl_scan<u64, 256>((u64)cnt, s_wave, block_total);
    if (cnt == 0) return;
    if (off + cnt > a.total) return;   // cannot happen: the lists hold exactly `total` pairs
    if (!a.brow_out) {   // SEMI / ANTI
        a.prow_out[off] = (u32)i;
        return;
    }
    const u32 first = a.first[i];
    if (first == kNone) {   // LEFT without a match
        a.prow_out[off] = (u32)i;
        a.brow_out[off] = kNone;
        return;
    }
    if (cnt == 1) {   // the common fact-to-dimension case: no second look at the key
        a.prow_out[off] = (u32)i;
        a.brow_out[off] = a.t.rows[first];
        return;
    }
    u64 img[4];
    key_images(a.kc, i, img);
    const u64 h = key_hash(img, a.kc.nkeys, a.t.mask);
    const u32 s1 = a.t.dir[(u32)(h >> (64 - a.t.dbits)) + 1];
    u32 found = 0;
    for (u32 s = first; s < s1 && found < cnt; ++s)
        if (entry_equal(a.t, s, img)) {
            a.prow_out[off + found] = (u32)i;
            a.brow_out[off + found] = a.t.rows[s];
            ++found;
        }
}

// RIGHT / FULL: matched -> unmatched, a lane per word; the last word keeps only the bits of real rows
__global__ void __launch_bounds__(256) join_unmatched_kernel(u64 *words, i64 n, i64 nwords) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 w = (i64)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride) {
        const i64 rem = n - w * 64;
        words[w] = ~words[w] & (rem < 64 ? (1ull << rem) - 1ull : ~0ull);
    }
}

inline unsigned capped_blocks(i64 n, i64 cap) {
    const i64 blocks = (n + 255) / 256;
    return (unsigned)(blocks < cap ? blocks : cap);
}

}  // namespace

void launch_join_build_keys(hipStream_t s, const JoinBuildArgs &a) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(join_build_keys_kernel, dim3(capped_blocks(a.n, 8192)), dim3(256), 0, s, a);
}

void launch_join_directory(hipStream_t s, const unsigned long long *sorted_hash, int64_t m, int dbits, uint32_t *dir) {
    const i64 nentries = (1ll << dbits) + 1;
    hipLaunchKernelGGL(join_directory_kernel, dim3(capped_blocks(nentries, 8192)), dim3(256), 0, s, (const u64 *)sorted_hash, (i64)m, dbits, dir, nentries);
}

int64_t join_probe_blocks(int64_t n) { return (n + 255) / 256; }

void launch_join_count(hipStream_t s, const JoinProbeArgs &a) {
    if (a.n <= 0) return;
    if (a.matched) hipLaunchKernelGGL(join_count_kernel<true>, dim3((unsigned)join_probe_blocks(a.n)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(join_count_kernel<false>, dim3((unsigned)join_probe_blocks(a.n)), dim3(256), 0, s, a);
}

void launch_join_write(hipStream_t s, const JoinProbeArgs &a) {
    if (a.n <= 0 || a.total == 0) return;
    hipLaunchKernelGGL(join_write_kernel, dim3((unsigned)join_probe_blocks(a.n)), dim3(256), 0, s, a);
}

void launch_join_unmatched(hipStream_t s, unsigned long long *words, int64_t n) {
    if (n <= 0) return;
    const i64 nwords = (n + 63) / 64;
    hipLaunchKernelGGL(join_unmatched_kernel, dim3(capped_blocks(nwords, 8192)), dim3(256), 0, s, (u64 *)words, (i64)n, nwords);
}

}  // namespace qe
