// qe_sort.cpp -- host side of the sorts (kernels: qe_sort.hip): the radix-sort scratch every sorting operator
// uses (RadixBuffers), the stable multi-key sort of a result's rows (SortDriver), that sort with the boundary flags of its
// runs (SortedRuns: the opening step of the window, the ordered-set aggregates, the set operations and the ASOF join), and
// ORDER BY itself with its top-k selection.
#include <algorithm>

#include "qe_exec.h"
#include "qe_kernels.h"
#include "qe_scan.h"

namespace qe {

RadixBuffers::RadixBuffers(PoolScratch &sc, int64_t m_, unsigned long long *keys0, uint32_t *rows0) : m(m_) {
    keys[0] = keys0 ? keys0 : (unsigned long long *)sc.alloc((size_t)m * 8);
    keys[1] = (unsigned long long *)sc.alloc((size_t)m * 8);
    rows[0] = rows0 ? rows0 : (uint32_t *)sc.alloc((size_t)m * 4);
    rows[1] = (uint32_t *)sc.alloc((size_t)m * 4);
    hist = (uint32_t *)sc.alloc((size_t)((m + 1023) / 1024) * 16 * 4);
}

void RadixBuffers::pass(hipStream_t s, int shift, const uint64_t *validity) {
    launch_radix_pass(s, keys[cur], rows[cur], validity, m, shift, hist, keys[cur ^ 1], rows[cur ^ 1]);
    cur ^= 1;
}

void SortDriver::prepare() {
    d_ranks.assign((size_t)nkeys, nullptr);
    nranks.assign((size_t)nkeys, 0);
    for (int32_t k = 0; k < nkeys; k++) {
        const OutColumn &kc = src->cols[(size_t)keys[k].column];
        if (kc.type != QE_STRING) continue;
        if (!kc.dict) fail(QE_ERR_INVALID_ARG, "STRING column without dictionary");
        // String.compareTo order of the dictionary (UTF-16 code units), as dense ranks
        h_ranks.push_back(merged_ranks({&kc.dict->entries}));
        const std::vector<int32_t> &ranks = h_ranks.back()[0];
        int *d = (int *)sc.alloc(ranks.size() * 4);
        if (!ranks.empty()) QE_HIP(hipMemcpyAsync(d, ranks.data(), ranks.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        d_ranks[(size_t)k] = d;
        nranks[(size_t)k] = (int)ranks.size();
    }
    if (!h_ranks.empty()) QE_HIP(hipStreamSynchronize(ctx->stream));
    d_bits = (unsigned long long *)sc.alloc(16);
}

void SortDriver::images(int32_t k, int64_t m, const uint32_t *perm, unsigned long long *keys_out, uint32_t *rows_out) {
    const OutColumn &kc = src->cols[(size_t)keys[k].column];
    SortKeyArgs ka{};
    ka.type = kc.type;
    ka.data = kc.data;
    ka.validity = (const unsigned long long *)kc.validity;
    ka.ranks = d_ranks[(size_t)k];
    ka.nranks = nranks[(size_t)k];
    ka.n = m;
    ka.keys = keys_out;
    ka.rows = rows_out;
    ka.perm = perm;
    ka.descending = keys[k].descending ? 1 : 0;
    launch_sort_keys(ctx->stream, ka);
}

unsigned long long SortDriver::varying(const unsigned long long *k, int64_t m) {
    const unsigned long long init[2] = {0ull, ~0ull};
    QE_HIP(hipMemcpyAsync(d_bits, init, 16, hipMemcpyHostToDevice, ctx->stream));
    launch_key_bits(ctx->stream, k, m, d_bits);
    unsigned long long h_bits[2] = {0, 0};
    QE_HIP(hipMemcpyAsync(h_bits, d_bits, 16, hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    return h_bits[0] & ~h_bits[1];
}

void SortDriver::sort(RadixBuffers &rb, bool identity) {
    for (int32_t k = nkeys - 1; k >= 0; k--) {
        const OutColumn &kc = src->cols[(size_t)keys[k].column];
        const bool first_sorted = identity && k == nkeys - 1;
        images(k, rb.m, first_sorted ? nullptr : rb.sorted_rows(), rb.sorted_keys(), rb.sorted_rows());
        const unsigned long long var = varying(rb.sorted_keys(), rb.m);
        for (int shift = 0; shift < 64; shift += 4) {
            if (((var >> shift) & 15ull) == 0) continue;   // the same digit in every key
            rb.pass(ctx->stream, shift);
            radix_passes++;
        }
        if (kc.validity) {   // NULL rows in front (compareValues) or, descending, behind; in their input order
            rb.pass(ctx->stream, keys[k].descending ? 65 : 64, kc.validity);
            radix_passes++;
        }
    }
}

SortedRuns::SortedRuns(qe_ctx *ctx, PoolScratch &ss, const qe_result *src, const qe_sort_key *keys, int32_t nkeys)
    : sorter{ctx, ss, src, keys, nkeys} {
    if (nkeys == 0) return;
    sorter.prepare();
    RadixBuffers rb(ss, src->count);
    sorter.sort(rb, true);
    rows = rb.sorted_rows();
}

void SortedRuns::flag(int32_t npart, unsigned long long *pstart, unsigned long long *peer, unsigned long long *counter) {
    WinFlagArgs fa{};
    fa.nkeys = sorter.nkeys;
    fa.npart = npart;
    fa.n = sorter.src->count;
    fa.pstart = pstart;
    fa.peer = peer;
    fa.npartitions = counter;
    fa.perm = rows;
    for (int32_t k = 0; k < sorter.nkeys; k++) {
        const OutColumn &kc = sorter.src->cols[(size_t)sorter.keys[k].column];
        fa.type[k] = kc.type;
        fa.data[k] = kc.data;
        fa.validity[k] = (const unsigned long long *)kc.validity;
        fa.ranks[k] = sorter.d_ranks[(size_t)k];
        fa.nranks[k] = sorter.nranks[(size_t)k];
    }
    QE_HIP(hipMemsetAsync(counter, 0, 16, sorter.ctx->stream));
    launch_win_flags(sorter.ctx->stream, fa);
}

void SortedRuns::rank_starts(const unsigned long long *pstart, uint32_t *prefix, uint32_t *sums) {
    bitmap_ranks(sorter.ctx->stream, (const uint64_t *)pstart, nullptr, sorter.src->count, prefix, sums, nullptr);
}

int64_t checked_runs(const char *who, unsigned long long count, const char *noun, int64_t n) {
    const int64_t G = (int64_t)count;
    if (G < 1 || G > n) fail(QE_ERR_INTERNAL, std::string(who) + ": " + std::to_string(G) + " " + noun + " of " + std::to_string(n) + " rows");
    return G;
}

// ORDER BY on the device: OrderByOperator.open (operator/OrderByOperator.kt:9-15) sorts the materialised rows stably
// with compareValues -- null first, Double.compareTo (-0.0 < 0.0, NaN greatest), String.compareTo (UTF-16 code units),
// false < true.  Key images + stable LSD radix sort of (key, row id) + gather of every column (qe_sort.hip).
//
// Several keys: the sort is stable, so it runs once per key from the LAST key to the first; the image of every key after
// the first one sorted is taken through the permutation reached so far, so the scratch stays two (u64, u32) buffers.  A
// descending key sorts the complement of its image and puts NULL last; ties keep their input order in both directions.
//
// LIMIT k (0 < k <= n / kTopkMaxShareDen; a larger k would make at least k rows candidates and goes straight to the full
// sort, truncated): radix select of the k-th smallest image of the FIRST key (NULL is the smallest image ascending and
// the greatest descending, so the NULL class is part of the order), the rows up to that threshold -- every tie of it
// included -- are compacted in row order, and only these c candidates go through the multi-key sort.  The first k sorted
// row ids are gathered.  When c exceeds n / kTopkMaxShareDen (a boolean or few-valued first key) the full sort runs instead.
namespace {

constexpr int64_t kTopkMaxShareDen = 2;       // candidates > n / 2: the full sort is taken (selection + the sort of c rows would cost as much)
constexpr int64_t kTopkStopFloor = 16384;     // the selection stops once this few rows are left (sorting them costs no more than one pass)

void order_by_impl(qe_ctx *ctx, const qe_result *src, const qe_sort_key *keys, int32_t nkeys, int64_t limit, const char *who, qe_result **out) {
    need_device(ctx);
    const int64_t n = src->count;
    if (n >= (1ll << 32)) fail(QE_ERR_UNSUPPORTED, std::string(who) + ": more than 2^32 rows");
    for (int32_t k = 0; k < nkeys; k++)
        if (keys[k].column < 0 || keys[k].column >= (int32_t)src->cols.size()) fail(QE_ERR_INVALID_ARG, std::string(who) + ": key column out of range");
    const int64_t nout = limit >= 0 && limit < n ? limit : n;
    ResultPtr res = new_result(ctx, nout);
    for (const OutColumn &c : src->cols) add_column(ctx, res.get(), c.type, c.validity != nullptr, c.dict, nout);
    int64_t stats[4] = {0, 0, 0, 0};
    if (nout > 0) {
        PoolScratch sc(ctx);
        SortDriver drv{ctx, sc, src, keys, nkeys};
        drv.prepare();
        unsigned long long *img = nullptr;   // top-k: the first key's images of every row
        uint32_t *cand = nullptr;            // .. and the candidate rows, in row order
        int64_t m = n;                       // rows that go into the sort
        if (nout < n && nout <= n / kTopkMaxShareDen) {
            // ---- top-k: select on the first key's images, candidates in row order ----
            img = (unsigned long long *)sc.alloc((size_t)n * 8);
            drv.images(0, n, nullptr, img, nullptr);
            const unsigned long long var = drv.varying(img, n);
            SelectState *st = (SelectState *)sc.alloc(sizeof(SelectState));
            SelectState init{};
            init.remaining = (unsigned long long)nout;
            QE_HIP(hipMemcpyAsync(st, &init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
            const unsigned long long stop_cap = (unsigned long long)std::max<int64_t>(nout + nout / 4, std::min<int64_t>(kTopkStopFloor, n / 16));
            for (int shift = 56; shift >= 0; shift -= 8) {
                if (((var >> shift) & 255ull) == 0) continue;   // the same digit in every key
                launch_select_pass(ctx->stream, img, n, shift, st, stop_cap);
            }
            const int64_t nblocks = select_compact_blocks(n);
            uint32_t *counts = (uint32_t *)sc.alloc((size_t)nblocks * 4), *offsets = (uint32_t *)sc.alloc((size_t)nblocks * 4);
            uint32_t *sums = (uint32_t *)sc.alloc((size_t)scan_blocks(nblocks) * 4);
            unsigned long long *d_total = (unsigned long long *)sc.alloc(16);
            launch_select_count(ctx->stream, img, n, st, counts);
            exclusive_scan<uint32_t>(ctx->stream, ArrayLoad<uint32_t>{counts}, offsets, sums, nblocks, d_total);
            unsigned long long c = 0;
            unsigned int passes = 0;
            QE_HIP(hipMemcpyAsync(&c, d_total, 8, hipMemcpyDeviceToHost, ctx->stream));   // the one read-back of the selection
            QE_HIP(hipMemcpyAsync(&passes, &st->passes, 4, hipMemcpyDeviceToHost, ctx->stream));
            QE_HIP(hipStreamSynchronize(ctx->stream));
            if ((int64_t)c < nout || (int64_t)c > n) fail(QE_ERR_INTERNAL, std::string(who) + ": top-k selection kept " + std::to_string(c) + " of " +
                                                                                std::to_string(n) + " rows for k = " + std::to_string(nout));
            stats[3] = passes;
            if ((int64_t)c <= n / kTopkMaxShareDen) {
                m = (int64_t)c;
                stats[0] = 1;
                cand = (uint32_t *)sc.alloc((size_t)m * 4);
                launch_select_compact(ctx->stream, img, n, st, counts, offsets, cand, m);
                img = nullptr;   // (n images: the sort of the m candidates takes buffers of its own size)
            }   // else too many candidates: the full sort, truncated, with the image buffer as its first key buffer
        }
        RadixBuffers rb(sc, m, img, cand);
        drv.sort(rb, cand == nullptr);
        stats[1] = m;
        stats[2] = drv.radix_passes;
        gather_columns(ctx, src->cols, rb.sorted_rows(), nout, res.get());
        QE_HIP(hipGetLastError());
        QE_HIP(hipStreamSynchronize(ctx->stream));
    }
    ctx->sort_stats.store(stats);
    *out = res.release();
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int32_t qe_result_order_by(qe_ctx *ctx, const qe_result *src, int32_t column, qe_result **out) {
    if (!ctx || !src || !out || column < 0 || column >= (int32_t)src->cols.size()) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    const qe_sort_key key{column, 0};
    return guarded(ctx, [&] { order_by_impl(ctx, src, &key, 1, -1, "qe_result_order_by", out); });
}

int32_t qe_result_order_by_keys(qe_ctx *ctx, const qe_result *src, const qe_sort_key *keys, int32_t nkeys, int64_t limit, qe_result **out) {
    if (out) *out = nullptr;
    if (!ctx || !src || !out || !keys || nkeys < 1 || nkeys > 8) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] { order_by_impl(ctx, src, keys, nkeys, limit, "qe_result_order_by_keys", out); });
}

int32_t qe_ctx_last_sort_stats(const qe_ctx *ctx, int64_t out[4]) { return last_stats(ctx, &qe_ctx::sort_stats, out); }

}  // extern "C"
