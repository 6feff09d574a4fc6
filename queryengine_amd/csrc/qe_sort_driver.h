// qe_sort_driver.h -- the stable multi-key sort of a result's rows as the files behind the C ABI share it:
// qe_comm.cpp (ORDER BY) and qe_window.cpp (the partition / order sort of the window operator).  Not part of the ABI.
#pragma once

#include <algorithm>
#include <vector>

#include "qe_internal.h"
#include "qe_kernels.h"

namespace qe {
#pragma GCC visibility push(hidden)

struct SortDriver {
    qe_ctx *ctx;
    PoolScratch &sc;
    const qe_result *src;
    const qe_sort_key *keys;
    int32_t nkeys;
    std::vector<const int *> d_ranks;   // per key: compareTo ranks of a STRING column's dictionary
    std::vector<int> nranks;
    std::vector<std::vector<std::vector<int32_t>>> h_ranks;   // the host tables, alive until the uploads have completed
    unsigned long long *d_bits = nullptr;
    int64_t radix_passes = 0;

    void prepare() {
        d_ranks.assign((size_t)nkeys, nullptr);
        nranks.assign((size_t)nkeys, 0);
        for (int32_t k = 0; k < nkeys; k++) {
            const OutColumn &kc = src->cols[(size_t)keys[k].column];
            if (kc.type != QE_STRING) continue;
            if (!kc.dict) fail(QE_ERR_INVALID_ARG, "STRING column without dictionary");
            // String.compareTo order of the dictionary (UTF-16 code units), as dense ranks
            h_ranks.push_back(merged_ranks({&kc.dict->entries}));
            const std::vector<int32_t> &ranks = h_ranks.back()[0];
            int *d = (int *)sc.alloc(std::max<size_t>(ranks.size() * 4, 16));
            if (!ranks.empty()) QE_HIP(hipMemcpyAsync(d, ranks.data(), ranks.size() * 4, hipMemcpyHostToDevice, ctx->stream));
            d_ranks[(size_t)k] = d;
            nranks[(size_t)k] = (int)ranks.size();
        }
        if (!h_ranks.empty()) QE_HIP(hipStreamSynchronize(ctx->stream));
        d_bits = (unsigned long long *)sc.alloc(16);
    }

    // images of key k for m elements: of rows 0..m-1 (perm == nullptr; rows_out[i] = i unless null) or of rows perm[0..m)
    void images(int32_t k, int64_t m, const uint32_t *perm, unsigned long long *keys_out, uint32_t *rows_out) {
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

    // bits that differ between the m images (a digit without such a bit is the same in every key: its pass is skipped)
    unsigned long long varying(const unsigned long long *k, int64_t m) {
        const unsigned long long init[2] = {0ull, ~0ull};
        QE_HIP(hipMemcpyAsync(d_bits, init, 16, hipMemcpyHostToDevice, ctx->stream));
        launch_key_bits(ctx->stream, k, m, d_bits);
        unsigned long long h_bits[2] = {0, 0};
        QE_HIP(hipMemcpyAsync(h_bits, d_bits, 16, hipMemcpyDeviceToHost, ctx->stream));
        QE_HIP(hipStreamSynchronize(ctx->stream));
        return h_bits[0] & ~h_bits[1];
    }

    // stable sort of the m row ids in rbuf[0] (identity: they are 0..m-1 and are written here) by all keys; the index of
    // the buffer that holds the sorted row ids is returned
    int sort(int64_t m, bool identity, unsigned long long *kbuf[2], uint32_t *rbuf[2], uint32_t *hist) {
        int cur = 0;
        for (int32_t k = nkeys - 1; k >= 0; k--) {
            const OutColumn &kc = src->cols[(size_t)keys[k].column];
            const bool first_sorted = identity && k == nkeys - 1;
            images(k, m, first_sorted ? nullptr : rbuf[cur], kbuf[cur], rbuf[cur]);
            const unsigned long long var = varying(kbuf[cur], m);
            for (int shift = 0; shift < 64; shift += 4) {
                if (((var >> shift) & 15ull) == 0) continue;   // the same digit in every key
                launch_radix_pass(ctx->stream, kbuf[cur], rbuf[cur], nullptr, m, shift, hist, kbuf[cur ^ 1], rbuf[cur ^ 1]);
                cur ^= 1;
                radix_passes++;
            }
            if (kc.validity) {   // NULL rows in front (compareValues) or, descending, behind; in their input order
                launch_radix_pass(ctx->stream, kbuf[cur], rbuf[cur], kc.validity, m, keys[k].descending ? 65 : 64, hist, kbuf[cur ^ 1], rbuf[cur ^ 1]);
                cur ^= 1;
                radix_passes++;
            }
        }
        return cur;
    }
};

// every column of `src` through the row ids rows[0 .. nout) into the first columns of `dst` (same types; a validity bitmap
// where dst carries one)
inline void gather_all_columns(qe_ctx *ctx, const qe_result *src, const uint32_t *rows, int64_t nout, qe_result *dst) {
    for (size_t c = 0; c < src->cols.size(); c++) {
        const OutColumn &s_ = src->cols[c];
        OutColumn &d_ = dst->cols[c];
        const int width = (s_.type == QE_DOUBLE || s_.type == QE_INT64) ? 8 : 4;
        if (s_.type == QE_BOOLEAN) launch_gather_bits_rows(ctx->stream, (const uint64_t *)s_.data, rows, nout, (uint64_t *)d_.data);
        else launch_gather_rows(ctx->stream, width, s_.data, rows, nout, d_.data);
        if (d_.nullable) launch_gather_bits_rows(ctx->stream, s_.validity, rows, nout, d_.validity);
    }
}

#pragma GCC visibility pop
}  // namespace qe
