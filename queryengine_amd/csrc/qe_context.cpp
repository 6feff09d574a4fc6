// qe_context.cpp -- errors, the device and pinned pools, and the entry points of include/qe_hip.h that own state rather than
// execute plans: contexts, dictionaries, HBM-resident batches, expression handles, the two stream calibrations.
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <sstream>

#include "qe_exec.h"
#include "qe_kernels.h"

namespace qe {

void fail(int32_t code, const std::string &msg) { throw Error{code, msg}; }

void hip_check(hipError_t e, const char *what, const char *file, int line) {
    if (e == hipSuccess) return;
    std::ostringstream s;
    s << what << " failed: " << hipGetErrorString(e) << " (" << (int)e << ") at " << file << ":" << line;
    fail(e == hipErrorOutOfMemory ? QE_ERR_OOM : QE_ERR_HIP, s.str());
}

uint64_t DictData::next_id() {
    static std::atomic<uint64_t> counter{0};
    return ++counter;
}

// ---- pool ------------------------------------------------------------------------------
// Every request is rounded up to whole 256-byte blocks, at least one: this is the ONE place that handles a zero-byte request
// (an empty column, a sort of no rows), so callers pass the size they mean.
void *Pool::alloc(size_t bytes) {
    bytes = std::max<size_t>(256, (bytes + 255) & ~size_t(255));
    auto it = free_.lower_bound(bytes);
    if (it != free_.end() && it->first <= bytes + bytes / 4) {
        void *p = it->second;
        bytes_cached -= it->first;
        bytes_in_use += it->first;
        live_[p] = it->first;
        free_.erase(it);
        return p;
    }
    void *p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipErrorOutOfMemory && !free_.empty()) {
        (void)hipGetLastError();
        trim_all();
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fail(QE_ERR_OOM, "hipMalloc of " + std::to_string(bytes) + " bytes failed: " + hipGetErrorString(e));
    }
    live_[p] = bytes;
    bytes_in_use += bytes;
    return p;
}

void Pool::release(void *p) {
    if (!p) return;
    auto it = live_.find(p);
    if (it == live_.end()) return;
    bytes_in_use -= it->second;
    bytes_cached += it->second;
    free_.emplace(it->second, p);
    live_.erase(it);
}

void Pool::trim_all() {
    for (auto &kv : free_) (void)hipFree(kv.second);
    free_.clear();
    bytes_cached = 0;
}
void Pool::trim() { trim_all(); }

void *PinnedPool::alloc(size_t bytes) {
    bytes = (std::max<size_t>(bytes, 64) + 4095) & ~(size_t)4095;
    auto it = free_.lower_bound(bytes);
    if (it != free_.end() && it->first <= bytes + bytes / 4 + (1u << 20)) {   // a cached buffer that is not wastefully large
        void *p = it->second;
        live_[p] = it->first;
        free_.erase(it);
        return p;
    }
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        trim();   // give the cached buffers back and try once more
        e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            fail(QE_ERR_OOM, "hipHostMalloc of " + std::to_string(bytes) + " bytes of pinned host memory failed: " + hipGetErrorString(e));
        }
    }
    live_[p] = bytes;
    return p;
}

void PinnedPool::release(void *p) {
    if (!p) return;
    auto it = live_.find(p);
    if (it == live_.end()) return;
    free_.emplace(it->second, p);
    live_.erase(it);
}

void PinnedPool::trim() {
    for (auto &kv : free_) (void)hipHostFree(kv.second);
    free_.clear();
}

}  // namespace qe

namespace qe {

std::string &error_slot(qe_ctx *ctx) {
    static thread_local std::string create_error;   // qe_ctx_create has no context to leave its message in
    return ctx ? ctx->last_error : create_error;
}

void need_device(const qe_ctx *ctx) {
    if (ctx->device < 0)
        fail(QE_ERR_HIP, "planning-only context (QE_DEVICE_NONE): this call needs a HIP device; libqe_hip has no CPU fallback");
    QE_HIP(hipSetDevice(ctx->device));
}

void free_batch(qe_ctx *ctx, qe_batch *b) {
    if (!b) return;
    for (auto &c : b->cols)
        if (c.owned) {
            ctx->pool.release(c.data);
            ctx->pool.release(c.validity);
        }
    if (qe_result *r = b->view_of)   // a view of a result: the last one to go releases a result that was freed meanwhile
        if (--r->views == 0 && r->free_pending) free_result(ctx, r);
    delete b;
}

}  // namespace qe

using namespace qe;

static std::string default_cache_dir() {
    if (const char *e = std::getenv("QE_JIT_CACHE_DIR")) return e;
    Dl_info info;
    if (dladdr((void *)&default_cache_dir, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        size_t s = p.rfind('/');
        if (s != std::string::npos) return p.substr(0, s) + "/jit_cache";
    }
    return "jit_cache";
}

extern "C" {

int32_t qe_abi_version(void) { return QE_ABI_VERSION; }

const char *qe_last_error(const qe_ctx *ctx) { return error_slot(const_cast<qe_ctx *>(ctx)).c_str(); }

int32_t qe_ctx_create(int32_t device, const qe_options *opts, qe_ctx **out) {
    if (!out) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    qe_ctx *ctx = nullptr;
    int32_t st = guarded(nullptr, [&] {
        if (device == QE_DEVICE_NONE) {   // planning-only context: no HIP call at all
            ctx = new qe_ctx();
            ctx->device = device;
            if (opts) std::memcpy(&ctx->opts, opts, std::min<size_t>(opts->struct_size, sizeof(qe_options)));
            ctx->opts.struct_size = sizeof(qe_options);
            ctx->jit.reset(new Jit(ctx->opts.jit_cache_dir ? ctx->opts.jit_cache_dir : default_cache_dir()));
            ctx->opts.jit_cache_dir = nullptr;
            return;
        }
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0) {
            (void)hipGetLastError();
            fail(QE_ERR_HIP, std::string("no HIP device available: ") + hipGetErrorString(e) +
                                 " (libqe_hip has no CPU fallback)");
        }
        if (device < 0 || device >= ndev) fail(QE_ERR_INVALID_ARG, "device ordinal out of range");
        ctx = new qe_ctx();
        ctx->device = device;
        if (opts) {
            size_t n = std::min<size_t>(opts->struct_size, sizeof(qe_options));
            std::memcpy(&ctx->opts, opts, n);
        }
        ctx->opts.struct_size = sizeof(qe_options);
        QE_HIP(hipSetDevice(device));
        QE_HIP(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        QE_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        QE_HIP(hipEventCreate(&ctx->ev0));
        QE_HIP(hipEventCreate(&ctx->ev1));
        QE_HIP(hipMalloc((void **)&ctx->d_ctrl, 256));
        QE_HIP(hipHostMalloc((void **)&ctx->h_ctrl, 256, hipHostMallocDefault));
        ctx->jit.reset(new Jit(ctx->opts.jit_cache_dir ? ctx->opts.jit_cache_dir : default_cache_dir()));
        ctx->opts.jit_cache_dir = nullptr;
    });
    if (st != QE_OK) {
        delete ctx;
        return st;
    }
    *out = ctx;
    return QE_OK;
}

void qe_ctx_destroy(qe_ctx *ctx) {
    if (!ctx) return;
    if (ctx->device < 0) {
        delete ctx;
        return;
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    while (!ctx->host_results.empty()) qe_host_result_free(ctx, ctx->host_results.back());
    ctx->pinned.trim();
    qe_comm_destroy(ctx);
    ctx->plans.clear();
    ctx->jit.reset();
    ctx->pool.trim();
    if (ctx->d_ctrl) (void)hipFree(ctx->d_ctrl);
    if (ctx->h_ctrl) (void)hipHostFree(ctx->h_ctrl);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    delete ctx;
}

int32_t qe_ctx_set_exec_mode(qe_ctx *ctx, int32_t m) {
    if (!ctx || (m != QE_EXEC_FUSED && m != QE_EXEC_PER_NODE)) return QE_ERR_INVALID_ARG;
    ctx->opts.exec_mode = m;
    return QE_OK;
}
int32_t qe_ctx_set_cmp_semantics(qe_ctx *ctx, int32_t m) {
    if (!ctx || (m != QE_CMP_TOTAL_ORDER && m != QE_CMP_IEEE)) return QE_ERR_INVALID_ARG;
    ctx->opts.cmp_semantics = m;
    return QE_OK;
}
int32_t qe_ctx_kernel_time(qe_ctx *ctx, double *last_ms, double *total_ms, int64_t *launches) {
    if (!ctx) return QE_ERR_INVALID_ARG;
    if (last_ms) *last_ms = ctx->last_ms;
    if (total_ms) *total_ms = ctx->total_ms;
    if (launches) *launches = ctx->launches;
    return QE_OK;
}
int32_t qe_ctx_reset_kernel_time(qe_ctx *ctx) {
    if (!ctx) return QE_ERR_INVALID_ARG;
    ctx->last_ms = ctx->total_ms = 0.0;
    ctx->launches = 0;
    return QE_OK;
}
int32_t qe_ctx_last_form(const qe_ctx *ctx) { return ctx ? ctx->last_form : -1; }
int32_t qe_ctx_synchronize(qe_ctx *ctx) {
    if (!ctx) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] { need_device(ctx); QE_HIP(hipStreamSynchronize(ctx->stream)); });
}
int32_t qe_ctx_trim(qe_ctx *ctx) {
    if (!ctx) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        need_device(ctx);
        QE_HIP(hipStreamSynchronize(ctx->stream));
        ctx->pool.trim();
        ctx->pinned.trim();
    });
}

// ---- dictionaries ---------------------------------------------------------------------------
int32_t qe_dict_create(qe_ctx *ctx, int32_t nentries, const char *const *utf8, qe_dict **out) {
    if (!ctx || !out || nentries < 0 || (nentries > 0 && !utf8)) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        auto d = std::make_shared<DictData>();
        d->entries.reserve(nentries);
        for (int32_t i = 0; i < nentries; i++) {
            if (!utf8[i]) fail(QE_ERR_INVALID_ARG, "null dictionary entry");
            d->entries.emplace_back(utf8[i]);
            d->index.emplace(d->entries.back(), i);   // first occurrence wins
        }
        *out = new qe_dict{d};
    });
}
int32_t qe_dict_size(const qe_dict *dict) { return dict && dict->d ? (int32_t)dict->d->entries.size() : 0; }
const char *qe_dict_entry(const qe_dict *dict, int32_t code) {
    if (!dict || !dict->d || code < 0 || code >= (int32_t)dict->d->entries.size()) return nullptr;
    return dict->d->entries[code].c_str();
}
void qe_dict_free(qe_ctx *, qe_dict *dict) { delete dict; }

// ---- batches ------------------------------------------------------------------------------------
static void check_col_desc(const qe_col_desc &d, int64_t nrows) {
    if (d.type < QE_STRING || d.type > QE_INT32) fail(QE_ERR_INVALID_ARG, "bad column type");
    if (nrows > 0 && !d.data) fail(QE_ERR_INVALID_ARG, "null column data");
    if (d.type == QE_STRING && (!d.dict || !d.dict->d)) fail(QE_ERR_INVALID_ARG, "STRING column needs a dictionary");
}

int32_t qe_batch_create(qe_ctx *ctx, int64_t nrows, int32_t ncols, const qe_col_desc *cols, qe_batch **out) {
    if (!ctx || !out || nrows < 0 || ncols < 0 || (ncols > 0 && !cols)) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    qe_batch *b = nullptr;
    int32_t st = guarded(ctx, [&] {
        need_device(ctx);
        b = new qe_batch();
        b->nrows = nrows;
        for (int32_t j = 0; j < ncols; j++) {
            check_col_desc(cols[j], nrows);
            Column c;
            c.type = cols[j].type;
            if (c.type == QE_STRING) c.dict = cols[j].dict->d;
            size_t nb = column_bytes(c.type, nrows);
            c.data = ctx->pool.alloc(nb);
            b->cols.push_back(c);
            if (nb) QE_HIP(hipMemcpyAsync(c.data, cols[j].data, nb, hipMemcpyHostToDevice, ctx->stream));
            if (cols[j].validity) {
                // also for an empty batch: nullability is part of the plan key, and the empty batch of a stream must find the
                // plan of its schema, not compile one for a schema without nulls
                b->cols.back().validity = (uint64_t *)ctx->pool.alloc(bitmap_bytes(nrows));
                if (nrows > 0)
                    QE_HIP(hipMemcpyAsync(b->cols.back().validity, cols[j].validity, bitmap_bytes(nrows),
                                          hipMemcpyHostToDevice, ctx->stream));
            }
        }
        QE_HIP(hipStreamSynchronize(ctx->stream));   // host buffers may be reused by the caller
    });
    if (st != QE_OK) {
        free_batch(ctx, b);
        return st;
    }
    *out = b;
    return QE_OK;
}

int32_t qe_batch_wrap_device(qe_ctx *ctx, int64_t nrows, int32_t ncols, const qe_col_desc *cols, qe_batch **out) {
    if (!ctx || !out || nrows < 0 || ncols < 0 || (ncols > 0 && !cols)) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    qe_batch *b = nullptr;
    int32_t st = guarded(ctx, [&] {
        b = new qe_batch();
        b->nrows = nrows;
        for (int32_t j = 0; j < ncols; j++) {
            check_col_desc(cols[j], nrows);
            if (((uintptr_t)cols[j].data & 15) || ((uintptr_t)cols[j].validity & 7))
                fail(QE_ERR_INVALID_ARG, "device column pointers must be 16-byte aligned (validity: 8)");
            Column c;
            c.type = cols[j].type;
            c.data = const_cast<void *>(cols[j].data);
            c.validity = const_cast<uint64_t *>(cols[j].validity);
            if (c.type == QE_STRING) c.dict = cols[j].dict->d;
            c.owned = false;
            b->cols.push_back(c);
        }
    });
    if (st != QE_OK) {
        delete b;
        return st;
    }
    *out = b;
    return QE_OK;
}

int32_t qe_batch_describe(qe_ctx *ctx, int64_t nrows, int32_t ncols, const qe_col_desc *cols, qe_batch **out) {
    if (!ctx || !out || nrows < 0 || ncols < 0 || (ncols > 0 && !cols)) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    qe_batch *b = nullptr;
    int32_t st = guarded(ctx, [&] {
        b = new qe_batch();
        b->nrows = nrows;
        b->schema_only = true;
        for (int32_t j = 0; j < ncols; j++) {
            if (cols[j].type < QE_STRING || cols[j].type > QE_INT32) fail(QE_ERR_INVALID_ARG, "bad column type");
            if (cols[j].type == QE_STRING && (!cols[j].dict || !cols[j].dict->d))
                fail(QE_ERR_INVALID_ARG, "STRING column needs a dictionary");
            Column c;
            c.type = cols[j].type;
            c.validity = cols[j].validity ? (uint64_t *)(uintptr_t)8 : nullptr;   // nullability marker only
            if (c.type == QE_STRING) c.dict = cols[j].dict->d;
            c.owned = false;
            b->cols.push_back(c);
        }
    });
    if (st != QE_OK) {
        delete b;
        return st;
    }
    *out = b;
    return QE_OK;
}

int32_t qe_batch_generate(qe_ctx *ctx, uint64_t seed, int64_t row_begin, int64_t nrows, int32_t ncols,
                          const qe_gen_spec *specs, qe_batch **out) {
    if (!ctx || !out || nrows < 0 || row_begin < 0 || ncols < 0 || (ncols > 0 && !specs)) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    qe_batch *b = nullptr;
    int32_t st = guarded(ctx, [&] {
        need_device(ctx);
        b = new qe_batch();
        b->nrows = nrows;
        for (int32_t j = 0; j < ncols; j++) {
            const qe_gen_spec &g = specs[j];
            Column c;
            switch (g.kind) {
            case QE_GEN_I64_MOD: case QE_GEN_I64_ROWID: c.type = QE_INT64; break;
            case QE_GEN_I32_MOD: c.type = QE_INT32; break;
            case QE_GEN_DICT_MOD:
                c.type = QE_STRING;
                if (!g.dict || !g.dict->d) fail(QE_ERR_INVALID_ARG, "QE_GEN_DICT_MOD needs a dictionary");
                if (g.modulus > g.dict->d->entries.size() || g.offset != 0)
                    fail(QE_ERR_INVALID_ARG, "QE_GEN_DICT_MOD codes exceed the dictionary");
                c.dict = g.dict->d;
                break;
            case QE_GEN_F64_UNIT: case QE_GEN_F64_MOD: case QE_GEN_F64_STEP: case QE_GEN_F64_PRICE: c.type = QE_DOUBLE; break;
            default: fail(QE_ERR_INVALID_ARG, "bad generator kind");
            }
            if (g.kind != QE_GEN_F64_UNIT && g.kind != QE_GEN_F64_PRICE && g.kind != QE_GEN_I64_ROWID && g.modulus == 0)
                fail(QE_ERR_INVALID_ARG, "generator modulus must be > 0");
            c.data = ctx->pool.alloc(column_bytes(c.type, nrows));
            if (g.null_pct > 0 && nrows > 0) c.validity = (uint64_t *)ctx->pool.alloc(bitmap_bytes(nrows));
            b->cols.push_back(c);
            launch_generate(ctx->stream, g, seed, row_begin, nrows, c.data, c.validity);
        }
        QE_HIP(hipGetLastError());
        QE_HIP(hipStreamSynchronize(ctx->stream));
    });
    if (st != QE_OK) {
        free_batch(ctx, b);
        return st;
    }
    *out = b;
    return QE_OK;
}

int64_t qe_batch_nrows(const qe_batch *b) { return b ? b->nrows : -1; }
int32_t qe_batch_ncols(const qe_batch *b) { return b ? (int32_t)b->cols.size() : -1; }
int32_t qe_batch_column_type(const qe_batch *b, int32_t col) {
    return (b && col >= 0 && col < (int32_t)b->cols.size()) ? b->cols[col].type : -1;
}
int32_t qe_batch_column_nullable(const qe_batch *b, int32_t col) {
    if (!b || col < 0 || col >= (int32_t)b->cols.size()) return -1;
    return b->cols[(size_t)col].validity ? 1 : 0;
}
int32_t qe_batch_column_dict(const qe_batch *b, int32_t col, qe_dict **out) {
    if (!b || !out || col < 0 || col >= (int32_t)b->cols.size() || !b->cols[(size_t)col].dict) return QE_ERR_INVALID_ARG;
    *out = new qe_dict{b->cols[(size_t)col].dict};
    return QE_OK;
}

int32_t qe_batch_column_to_host(qe_ctx *ctx, const qe_batch *b, int32_t col, int64_t row_begin, int64_t nrows,
                                void *data_out, uint64_t *validity_out) {
    if (!ctx || !b || col < 0 || col >= (int32_t)b->cols.size() || row_begin < 0 || nrows < 0 ||
        row_begin + nrows > b->nrows || (row_begin & 63))
        return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        need_device(ctx);
        const Column &c = b->cols[col];
        if (nrows == 0) return;
        if (data_out) {
            if (c.type == QE_BOOLEAN)
                QE_HIP(hipMemcpyAsync(data_out, (const char *)c.data + (row_begin / 64) * 8, bitmap_bytes(nrows),
                                      hipMemcpyDeviceToHost, ctx->stream));
            else
                QE_HIP(hipMemcpyAsync(data_out, (const char *)c.data + type_width(c.type) * (size_t)row_begin,
                                      type_width(c.type) * (size_t)nrows, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (validity_out) {
            if (c.validity)
                QE_HIP(hipMemcpyAsync(validity_out, c.validity + row_begin / 64, bitmap_bytes(nrows),
                                      hipMemcpyDeviceToHost, ctx->stream));
            else
                std::memset(validity_out, 0xff, bitmap_bytes(nrows));
        }
        QE_HIP(hipStreamSynchronize(ctx->stream));
    });
}

void qe_batch_free(qe_ctx *ctx, qe_batch *b) {
    if (!ctx) return;
    free_batch(ctx, b);
}

// ---- expressions ---------------------------------------------------------------------------------
int32_t qe_expr_compile(qe_ctx *ctx, const uint8_t *program, size_t len, qe_expr **out) {
    if (!ctx || !out) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    return guarded(ctx, [&] {
        Expr e = decode_program(program, len);
        *out = new qe_expr{std::move(e)};
    });
}
int32_t qe_expr_result_type(const qe_expr *e) { return e ? e->e.nodes[e->e.root].type : -1; }
void qe_expr_free(qe_ctx *, qe_expr *e) { delete e; }


int32_t qe_stream_read_write_time(qe_ctx *ctx, int64_t nbytes, int32_t write_every, int32_t reps, double *out_ms,
                                  double *out_written_bytes) {
    if (!ctx || nbytes < 4096 || reps < 1 || !out_ms) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        need_device(ctx);
        // write_every packs: [write_every % 1000] + 1000 * window_period_us + 1e7 * window_len_us
        const int we = write_every % 1000;
        const int64_t dst_bytes = we > 0 ? nbytes / 16 / we + (1 << 22) : (1 << 22);
        PoolScratch scratch(ctx);
        void *buf = scratch.alloc((size_t)nbytes);
        void *dst = scratch.alloc((size_t)dst_bytes);
        QE_HIP(hipMemsetAsync(buf, 0x5a, (size_t)nbytes, ctx->stream));
        double best = 1e30;
        for (int r = 0; r <= reps; r++) {
            QE_HIP(hipEventRecord(ctx->ev0, ctx->stream));
            launch_stream_read_write(ctx->stream, buf, nbytes, (unsigned long long *)(ctx->d_ctrl + 8), dst, dst_bytes,
                                     write_every % 1000, ((write_every / 1000) % 10000) * 100, (write_every / 10000000) * 100,
                                     std::getenv("QE_CALIB_BLOCKS") ? std::atoi(std::getenv("QE_CALIB_BLOCKS")) : 1);
            QE_HIP(hipEventRecord(ctx->ev1, ctx->stream));
            QE_HIP(hipStreamSynchronize(ctx->stream));
            float ms = 0.f;
            QE_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
            if (r > 0) best = std::min(best, (double)ms);
        }
        *out_ms = best;
        if (out_written_bytes) {
            // iterations per wave = nvec / (8 * threads); one 512-byte block per write_every iterations
            const double iters = (double)(nbytes / 16) / (8.0 * 256 * 8 * 256);
            *out_written_bytes = we > 0 ? std::floor(iters / we) * 512.0 * (256 * 8 * 4) : 0.0;
        }
    });
}

int32_t qe_stream_read_bandwidth(qe_ctx *ctx, int64_t nbytes, int32_t reps, double *out_gbps) {
    if (!ctx || nbytes < 4096 || reps < 1 || !out_gbps) return QE_ERR_INVALID_ARG;
    return guarded(ctx, [&] {
        need_device(ctx);
        PoolScratch scratch(ctx);
        void *buf = scratch.alloc((size_t)nbytes);
        QE_HIP(hipMemsetAsync(buf, 0x5a, (size_t)nbytes, ctx->stream));
        launch_stream_read(ctx->stream, buf, nbytes, (unsigned long long *)(ctx->d_ctrl + 8));
        QE_HIP(hipStreamSynchronize(ctx->stream));
        double best = 1e30;
        // the achievable read rate depends on how many waves stream: 8 per CU (2 workgroups) reach ~7 TB/s where 32 reach ~6.3
        // (tools/copy_calib.hip) -- the calibration reports the best of 2 / 4 / 8 workgroups per CU
        for (int wgs : {2, 4, 8}) {
            for (int r = 0; r < reps; r++) {
                QE_HIP(hipEventRecord(ctx->ev0, ctx->stream));
                launch_stream_read(ctx->stream, buf, nbytes, (unsigned long long *)(ctx->d_ctrl + 8), wgs);
                QE_HIP(hipEventRecord(ctx->ev1, ctx->stream));
                QE_HIP(hipStreamSynchronize(ctx->stream));
                float ms = 0.f;
                QE_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
                best = std::min(best, (double)ms);
            }
        }
        *out_gbps = (double)(nbytes / 16 * 16) / (best * 1e-3) / 1e9;
    });
}

}  // extern "C"
