// qe_result.cpp -- results: how the operators build one (new_result, add_column, gather_columns), their columns on the
// device (qe_result_*) and their way to the host, into a caller's pageable buffer (qe_result_column_to_host) or into pinned
// memory on the copy stream (qe_result_to_host, qe_host_result_*).
#include <algorithm>
#include <thread>

#include "qe_exec.h"
#include "qe_kernels.h"

namespace qe {

void free_result(qe_ctx *ctx, qe_result *r) {
    if (!r) return;
    for (auto &c : r->cols) {
        if (c.hold_data || c.hold_valid) {   // per-node results share buffers with pool-backed temporaries
            c.hold_data.reset();
            c.hold_valid.reset();
            continue;
        }
        ctx->pool.release(c.data);
        ctx->pool.release(c.validity);
        ctx->pool.release(c.bytes_data);
        ctx->pool.release(c.bytes_valid);
    }
    delete r;
}

ResultPtr new_result(qe_ctx *ctx, int64_t count) {
    ResultPtr res = own_result(ctx, new qe_result());
    res->count = res->capacity = count;
    return res;
}

OutColumn &add_column(qe_ctx *ctx, qe_result *res, int type, bool nullable, const std::shared_ptr<DictData> &dict, int64_t nrows) {
    res->cols.emplace_back();
    OutColumn &oc = res->cols.back();
    oc.type = type;
    oc.nullable = nullable;
    oc.dict = dict;
    oc.dict_handle.d = dict;
    oc.data = ctx->pool.alloc(column_bytes(type, nrows));
    if (nullable) oc.validity = (uint64_t *)ctx->pool.alloc(bitmap_bytes(nrows));
    return oc;
}

void drop_validity(qe_ctx *ctx, OutColumn &c) {
    ctx->pool.release(c.validity);
    c.validity = nullptr;
    c.nullable = false;
}

void gather_column(qe_ctx *ctx, int type, const void *data, const uint64_t *validity, const uint32_t *rows, int64_t nout, OutColumn &dst,
                   int max_blocks) {
    if (type == QE_BOOLEAN) launch_gather_bits_rows(ctx->stream, (const uint64_t *)data, rows, nout, (uint64_t *)dst.data, max_blocks);
    else launch_gather_rows(ctx->stream, (int)type_width(type), data, rows, nout, dst.data, max_blocks);
    if (dst.nullable) launch_gather_bits_rows(ctx->stream, validity, rows, nout, dst.validity, max_blocks);
}

void gather_columns(qe_ctx *ctx, const std::vector<OutColumn> &src_cols, const uint32_t *rows, int64_t nout, qe_result *dst) {
    for (size_t c = 0; c < src_cols.size(); c++)
        gather_column(ctx, src_cols[c].type, src_cols[c].data, src_cols[c].validity, rows, nout, dst->cols[c], kGatherBlocks);
}

}  // namespace qe

using namespace qe;

extern "C" {

// ---- results ----------------------------------------------------------------------------------------
int64_t qe_result_count(const qe_result *r) { return r ? r->count : -1; }
int32_t qe_result_ncols(const qe_result *r) { return r ? (int32_t)r->cols.size() : -1; }

int32_t qe_result_column(const qe_result *r, int32_t col, qe_col_view *out) {
    if (!r || !out || col < 0 || col >= (int32_t)r->cols.size()) return QE_ERR_INVALID_ARG;
    const OutColumn &c = r->cols[col];
    out->type = c.type;
    out->nullable = c.nullable ? 1 : 0;
    out->data = c.data;
    out->validity = c.validity;
    out->count = r->count;
    out->dict = c.dict ? &c.dict_handle : nullptr;
    return QE_OK;
}

// Device -> a caller's PAGEABLE buffer.  One hipMemcpy into pageable memory ran at 7 GB/s here (0.8 GB in 108 ms) while the
// link does ~55 GB/s into pinned memory: the bytes go through two pinned staging chunks on the copy stream, and the chunk
// that has arrived is copied into the caller's buffer (by a few host threads: one memcpy thread does ~10 GB/s) while the
// next one is on the link.
static void parallel_memcpy(void *dst, const void *src, size_t n) {
    const size_t kMin = 4u << 20;
    unsigned nthr = (unsigned)std::min<size_t>(4, n / kMin);
    if (nthr <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> ts;
    const size_t per = (((n + nthr - 1) / nthr) + 4095) & ~(size_t)4095;   // rounded up twice: nthr * per >= n
    for (unsigned t = 1; t < nthr; t++) {
        const size_t off = (size_t)t * per;
        if (off >= n) break;
        const size_t len = std::min(per, n - off);
        ts.emplace_back([=] { std::memcpy((char *)dst + off, (const char *)src + off, len); });
    }
    std::memcpy(dst, src, std::min(per, n));
    for (auto &t : ts) t.join();
}

static void staged_d2h(qe_ctx *ctx, void *dst, const void *src, size_t n) {
    const size_t kChunk = 32u << 20;
    if (n <= (1u << 20)) {   // small: not worth the staging
        QE_HIP(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, ctx->copy_stream));
        QE_HIP(hipStreamSynchronize(ctx->copy_stream));
        return;
    }
    void *stage[2] = {ctx->pinned.alloc(std::min(n, kChunk)), ctx->pinned.alloc(std::min(n, kChunk))};
    struct G { qe_ctx *c; void **s; ~G() { c->pinned.release(s[0]); c->pinned.release(s[1]); } } g{ctx, stage};
    hipEvent_t ev[2];
    QE_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
    QE_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
    struct EG { hipEvent_t *e; ~EG() { (void)hipEventDestroy(e[0]); (void)hipEventDestroy(e[1]); } } eg{ev};
    const size_t nchunks = (n + kChunk - 1) / kChunk;
    auto issue = [&](size_t k) {
        const size_t off = k * kChunk, len = std::min(kChunk, n - off);
        QE_HIP(hipMemcpyAsync(stage[k & 1], (const char *)src + off, len, hipMemcpyDeviceToHost, ctx->copy_stream));
        QE_HIP(hipEventRecord(ev[k & 1], ctx->copy_stream));
    };
    issue(0);
    for (size_t k = 0; k < nchunks; k++) {
        if (k + 1 < nchunks) issue(k + 1);
        QE_HIP(hipEventSynchronize(ev[k & 1]));
        const size_t off = k * kChunk, len = std::min(kChunk, n - off);
        parallel_memcpy((char *)dst + off, stage[k & 1], len);
    }
}

int32_t qe_result_column_to_host(qe_ctx *ctx, const qe_result *r, int32_t col, void *data_out, uint64_t *validity_out) {
    if (!ctx || !r || col < 0 || col >= (int32_t)r->cols.size()) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        need_device(ctx);
        const OutColumn &c = r->cols[col];
        if (r->count == 0) return;
        if (data_out) staged_d2h(ctx, data_out, c.data, column_bytes(c.type, r->count));
        if (validity_out) {
            if (c.validity) staged_d2h(ctx, validity_out, c.validity, bitmap_bytes(r->count));
            else std::memset(validity_out, 0xff, bitmap_bytes(r->count));
        }
    });
}

// Result -> PINNED host memory owned by the library, on the context's copy stream: the call returns at once, so the scan of
// the next batch (compute stream) runs beside the copy; qe_host_result_wait blocks until the bytes are there.  What a host
// that materialises rows (Main.kt:18 `physicalPlan.map { it }`, Operators.kt:5-11) reads them from -- no second copy.
int32_t qe_result_to_host(qe_ctx *ctx, const qe_result *r, qe_host_result **out) {
    if (!ctx || !r || !out) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(ctx, [&] {
        need_device(ctx);
        std::unique_ptr<qe_host_result> h(new qe_host_result());
        h->count = r->count;
        try {
            for (const OutColumn &c : r->cols) {
                qe_host_result::Col hc;
                hc.type = c.type;
                hc.nullable = c.validity != nullptr;
                hc.dict = c.dict;
                hc.dict_handle.d = c.dict;
                h->cols.push_back(hc);
                qe_host_result::Col &d = h->cols.back();
                d.data = ctx->pinned.alloc(column_bytes(c.type, r->count));
                if (c.validity) d.validity = (uint64_t *)ctx->pinned.alloc(bitmap_bytes(r->count));
            }
            QE_HIP(hipEventCreateWithFlags(&h->done, hipEventDisableTiming));
            if (r->count > 0) {
                for (size_t i = 0; i < r->cols.size(); i++) {
                    const OutColumn &c = r->cols[i];
                    QE_HIP(hipMemcpyAsync(h->cols[i].data, c.data, column_bytes(c.type, r->count), hipMemcpyDeviceToHost, ctx->copy_stream));
                    if (c.validity)
                        QE_HIP(hipMemcpyAsync(h->cols[i].validity, c.validity, bitmap_bytes(r->count), hipMemcpyDeviceToHost, ctx->copy_stream));
                }
            }
            QE_HIP(hipEventRecord(h->done, ctx->copy_stream));
        } catch (...) {
            (void)hipStreamSynchronize(ctx->copy_stream);
            for (auto &c : h->cols) {
                ctx->pinned.release(c.data);
                ctx->pinned.release(c.validity);
            }
            if (h->done) (void)hipEventDestroy(h->done);
            throw;
        }
        h->src = r;
        ctx->host_results.push_back(h.get());
        *out = h.release();
    });
}

int32_t qe_host_result_wait(qe_ctx *ctx, qe_host_result *h) {
    if (!ctx || !h) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        if (h->waited) return;
        QE_HIP(hipEventSynchronize(h->done));
        h->waited = true;
        h->src = nullptr;
    });
}

int64_t qe_host_result_count(const qe_host_result *h) { return h ? h->count : -1; }
int32_t qe_host_result_ncols(const qe_host_result *h) { return h ? (int32_t)h->cols.size() : -1; }

int32_t qe_host_result_column(const qe_host_result *h, int32_t col, qe_col_view *out) {
    if (!h || !out || col < 0 || col >= (int32_t)h->cols.size()) return QE_ERR_INVALID_ARG;
    const qe_host_result::Col &c = h->cols[col];
    out->type = c.type;
    out->nullable = c.nullable ? 1 : 0;
    out->data = c.data;
    out->validity = c.validity;
    out->count = h->count;
    out->dict = c.type == QE_STRING ? &c.dict_handle : nullptr;
    return QE_OK;
}

void qe_host_result_free(qe_ctx *ctx, qe_host_result *h) {
    if (!ctx || !h) return;
    if (!h->waited && h->done) (void)hipEventSynchronize(h->done);   // the copies write into the buffers released below
    for (auto &c : h->cols) {
        ctx->pinned.release(c.data);
        ctx->pinned.release(c.validity);
    }
    if (h->done) (void)hipEventDestroy(h->done);
    auto &v = ctx->host_results;
    v.erase(std::remove(v.begin(), v.end(), h), v.end());
    delete h;
}

void qe_result_free(qe_ctx *ctx, qe_result *r) {
    if (!ctx) return;
    // a copy to the host that still reads this result must finish before its buffers go back to the pool
    for (qe_host_result *h : ctx->host_results)
        if (h->src == r) {
            if (h->done) (void)hipEventSynchronize(h->done);
            h->waited = true;
            h->src = nullptr;
        }
    if (r && r->views > 0) {   // a batch of qe_batch_from_result still reads the buffers: its qe_batch_free releases them
        r->free_pending = true;
        return;
    }
    free_result(ctx, r);
}

}  // extern "C"
