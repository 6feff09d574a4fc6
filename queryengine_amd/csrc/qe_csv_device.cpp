// qe_csv_device.cpp -- host side of the device CSV parser (kernels: qe_csv_device.hip): CSV text -> qe_batch.
//
// The host resolves the header (the first non-empty record, through the host parser's header_fields) and copies the text
// after it to HBM through pinned staging.  Then the device passes run, one named step each: record starts, field spans, and
// per projected column the DOUBLE, BOOLEAN or STRING conversion.  Two of them bring field bytes back to the host, both through
// pack_fields: the distinct strings of a STRING column become its dictionary, and the DOUBLE fields that the device's
// converter leaves undecided are converted by the host's and scattered into the column.
// Whatever the device cannot prove it reads as the host does (a quote against the rule of the structure pass, an unterminated
// quote, a field that is no number) sends the whole input through the host parser + qe_csv_pin: same result or the same error.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <functional>
#include <thread>

#include "qe_exec.h"
#include "qe_scan.h"

namespace qe {
namespace {

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

// n elements of T among the device buffers of one call (PoolScratch returns them to the context's pool on every exit)
template <typename T>
T *dev_array(PoolScratch &S, size_t n) { return (T *)S.alloc(n * sizeof(T)); }

// exclusive sum of a[0..n) in place; a must hold n + 1 elements, a[n] = 0 on entry: the total lands in a[n]
void scan(qe_ctx *ctx, PoolScratch &S, i64 *a, i64 n) {
    exclusive_scan<i64>(ctx->stream, ArrayLoad<i64>{a}, a, dev_array<i64>(S, (size_t)scan_blocks(n + 1)), n + 1, nullptr);
}

template <typename T>
T read_back(qe_ctx *ctx, const T *dev) {
    T v{};
    QE_HIP(hipMemcpyAsync(&v, dev, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    QE_HIP(hipStreamSynchronize(ctx->stream));
    return v;
}

struct FallBack {};   // the device cannot prove its reading equal to the host parser's: the host parses the input

struct Request {
    int32_t nfields;
    const char *const *names;
    const int32_t *types;
};

// The header in the first n bytes: idx[k] = field of name k, body = where the text after it begins.  Returns false where the
// host parser would fail (no header, a missing name, a malformed quoted field, a bad type) -- its error text is the host's.
bool resolve_header(const char *data, size_t n, const Request &rq, size_t &body, std::vector<int> &idx) {
    for (int32_t k = 0; k < rq.nfields; k++) {
        if (!rq.names[k]) return false;
        if (rq.types[k] != QE_STRING && rq.types[k] != QE_DOUBLE && rq.types[k] != QE_BOOLEAN) return false;
    }
    try {
        idx = header_fields(data, n, body, rq.names, rq.nfields);
    } catch (const Error &) {
        return false;
    }
    return std::find(idx.begin(), idx.end(), -1) == idx.end();
}

// ---- the text and its way to HBM -----------------------------------------------------------------------------------------
struct TextSource {
    size_t nbytes = 0;         // of the whole text, known once open() has returned
    virtual ~TextSource() {}
    virtual void open() {}
    virtual std::pair<const char *, size_t> head() = 0;          // its first bytes: where the header is looked for
    virtual void read_at(char *dst, size_t off, size_t n) = 0;   // bytes [off, off + n): exactly n or throws; from several threads
};

struct MemSource : TextSource {
    const char *p;
    MemSource(const char *q, size_t n) : p(q) { nbytes = n; }
    std::pair<const char *, size_t> head() override { return {p, nbytes}; }
    void read_at(char *dst, size_t off, size_t n) override { std::memcpy(dst, p + off, n); }
};

struct FileSource : TextSource {
    const char *path;
    int fd = -1;
    std::vector<char> window;
    explicit FileSource(const char *s) : path(s) {}
    ~FileSource() override { if (fd >= 0) ::close(fd); }
    void open() override {
        fd = ::open(path, O_RDONLY);
        if (fd < 0) fail(QE_ERR_INVALID_ARG, std::string("cannot open ") + path + ": " + std::strerror(errno));
        struct stat sb;
        if (::fstat(fd, &sb) != 0) fail(QE_ERR_INVALID_ARG, std::string("read error on ") + path);
        nbytes = (size_t)sb.st_size;
    }
    // the header from the first 1 MiB; a header that does not end there goes the host's way
    std::pair<const char *, size_t> head() override {
        window = std::vector<char>(std::min<size_t>(nbytes, (size_t)1 << 20));
        if (!window.empty()) read_at(window.data(), 0, window.size());
        return {window.data(), window.size()};
    }
    void read_at(char *dst, size_t off, size_t n) override {
        while (n > 0) {
            const ssize_t r = ::pread(fd, dst, n, (off_t)off);
            if (r <= 0) {
                if (r < 0 && errno == EINTR) continue;
                fail(QE_ERR_INVALID_ARG, std::string("read error on ") + path);
            }
            dst += r; off += (size_t)r; n -= (size_t)r;
        }
    }
};

// Fill a chunk with a few host threads: one memcpy / pread thread moves ~10 GB/s, the link ~55 GB/s.
void parallel_read(TextSource &src, char *dst, size_t off, size_t n) {
    const size_t kMin = 4u << 20;
    const unsigned nthr = (unsigned)std::min<size_t>(8, std::max<size_t>(1, n / kMin));
    if (nthr <= 1) {
        src.read_at(dst, off, n);
        return;
    }
    // whole pages per thread, rounded UP twice: n / nthr rounded down leaves the last n % nthr bytes to nobody when it is a
    // whole number of pages already
    const size_t per = (((n + nthr - 1) / nthr) + 4095) & ~(size_t)4095;
    std::vector<std::thread> ts;
    std::vector<std::string> errs(nthr);
    for (unsigned t = 1; t < nthr; t++) {
        const size_t o = (size_t)t * per;
        if (o >= n) break;
        const size_t len = std::min(per, n - o);
        ts.emplace_back([&, t, o, len] {
            try { src.read_at(dst + o, off + o, len); } catch (const Error &e) { errs[t] = e.msg.empty() ? "read error" : e.msg; }
        });
    }
    try { src.read_at(dst, off, std::min(per, n)); } catch (const Error &e) { errs[0] = e.msg.empty() ? "read error" : e.msg; }
    for (auto &t : ts) t.join();
    for (auto &e : errs)
        if (!e.empty()) fail(QE_ERR_INVALID_ARG, e);
}

// bytes [body, body + n) of the text -> HBM through two pinned chunks: the fill of one runs beside the copy of the other
void upload(qe_ctx *ctx, TextSource &src, size_t body, unsigned char *dev, size_t n) {
    if (n == 0) return;
    const size_t chunk = (size_t)64 << 20;
    char *pin[2] = {(char *)ctx->pinned.alloc(std::min(chunk, n)), nullptr};
    struct Rel { qe_ctx *c; char **p; ~Rel() { c->pinned.release(p[0]); c->pinned.release(p[1]); } } rel{ctx, pin};
    if (n > chunk) pin[1] = (char *)ctx->pinned.alloc(chunk);
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct EvRel { hipEvent_t *e; ~EvRel() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evrel{ev};
    QE_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
    QE_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
    bool used[2] = {false, false};
    for (size_t off = 0, k = 0; off < n; off += chunk, k++) {
        const int b = (int)(k & 1);
        const size_t m = std::min(chunk, n - off);
        if (used[b]) QE_HIP(hipEventSynchronize(ev[b]));   // the copy out of this chunk two steps ago has finished
        parallel_read(src, pin[b], body + off, m);
        QE_HIP(hipMemcpyAsync(dev + off, pin[b], m, hipMemcpyHostToDevice, ctx->stream));
        QE_HIP(hipEventRecord(ev[b], ctx->stream));
        used[b] = true;
    }
    QE_HIP(hipStreamSynchronize(ctx->stream));
}

unsigned char *alloc_text(qe_ctx *ctx, PoolScratch &S, size_t n) {
    const size_t padded = ((n + kCsvTile - 1) / kCsvTile) * kCsvTile + 64;
    void *p = nullptr;
    try {
        p = dev_array<unsigned char>(S, padded);
    } catch (const Error &e) {
        fail(QE_ERR_OOM, "CSV text of " + std::to_string(n) + " bytes does not fit in free device memory (" + e.msg + ")");
    }
    QE_HIP(hipMemsetAsync((char *)p + n, 0, padded - n, ctx->stream));   // the passes read whole tiles
    return (unsigned char *)p;
}

// ---- the device passes -----------------------------------------------------------------------------------------------------
struct BatchDeleter {
    qe_ctx *ctx;
    void operator()(qe_batch *b) const { free_batch(ctx, b); }
};

// the unescaped bytes of a list of fields, back to back: field i is bytes[off[i], off[i + 1])
struct PackedFields {
    std::vector<i64> off;
    std::string bytes;
};

// The passes over one text, a step each, in the order parse_on_device takes them.  A step throws FallBack where the host
// parser has to decide.
struct Passes {
    qe_ctx *ctx;
    PoolScratch &S;
    const unsigned char *text;   // n bytes, padded with zeros to whole tiles
    i64 n;
    hipStream_t st;
    u32 *flags;                  // QE_CSV_*
    i64 nrows = 0;
    i64 *begin = nullptr;        // the field spans of all columns, column k at k * nrows
    u32 *lenesc = nullptr;
    u32 *any_null = nullptr;     // per column
    u32 *patch_count = nullptr, patch_cap = 0;
    i64 *patch_rows = nullptr;   // the rows of one DOUBLE column that the host converts

    Passes(qe_ctx *c, PoolScratch &s, const unsigned char *dev, i64 nbytes) : ctx(c), S(s), text(dev), n(nbytes), st(c->stream) {
        flags = dev_array<u32>(S, 4);
        QE_HIP(hipMemsetAsync(flags, 0, 16, st));
    }
    CsvFields fields(int k) const { return CsvFields{text, nrows, begin + (size_t)k * nrows, lenesc + (size_t)k * nrows}; }

    // 1 + 2: nrows and the first byte of every non-empty record, in row order
    const i64 *record_starts() {
        const i64 ntiles = (n + kCsvTile - 1) / kCsvTile;
        if (ntiles == 0) return nullptr;
        i64 *tq = dev_array<i64>(S, (size_t)ntiles + 1);
        QE_HIP(hipMemsetAsync(tq + ntiles, 0, sizeof(i64), st));
        launch_csv_quote_count(st, text, ntiles, tq);
        scan(ctx, S, tq, ntiles);
        if (read_back(ctx, tq + ntiles) & 1) throw FallBack{};   // an unterminated quote
        i64 *tr = dev_array<i64>(S, (size_t)ntiles + 1);
        QE_HIP(hipMemsetAsync(tr + ntiles, 0, sizeof(i64), st));
        launch_csv_records(st, false, text, n, ntiles, tq, tr, nullptr, flags);
        scan(ctx, S, tr, ntiles);
        nrows = read_back(ctx, tr + ntiles);
        if (read_back(ctx, flags) & QE_CSV_QUOTE_RULE) throw FallBack{};
        if (nrows >= (i64)0x7FFFFFFF) throw FallBack{};   // row ids of the dictionary table are 32-bit
        i64 *rec_start = dev_array<i64>(S, (size_t)nrows + 1);
        launch_csv_records(st, true, text, n, ntiles, tq, tr, rec_start, flags);
        return rec_start;
    }

    // 3: the span of every projected field; idx[k] = field of column k in a record
    void field_spans(const i64 *rec_start, const std::vector<int> &idx) {
        const int ncols = (int)idx.size();
        if (nrows == 0 || ncols == 0) return;
        begin = dev_array<i64>(S, (size_t)ncols * nrows);
        lenesc = dev_array<u32>(S, (size_t)ncols * nrows);
        int *field_of = dev_array<int>(S, (size_t)ncols);
        QE_HIP(hipMemcpyAsync(field_of, idx.data(), sizeof(int) * ncols, hipMemcpyHostToDevice, st));
        launch_csv_spans(st, CsvSpanArgs{fields(0), n, rec_start, field_of, ncols, *std::max_element(idx.begin(), idx.end())});
    }

    // what the column steps share: the NULL flags and the patch list
    void begin_columns(int ncols) {
        any_null = dev_array<u32>(S, (size_t)std::max(ncols, 1));
        QE_HIP(hipMemsetAsync(any_null, 0, sizeof(u32) * std::max(ncols, 1), st));
        patch_count = dev_array<u32>(S, 1);
        patch_cap = (u32)std::min<i64>(std::max<i64>(nrows, 1), 1 << 20);
        patch_rows = dev_array<i64>(S, patch_cap);
    }

    // one more column of the batch, its buffers sized like qe_batch_create's (pushed first: the batch owns whatever is allocated)
    Column &add_column(qe_batch *b, int type) {
        Column blank;
        blank.type = type;
        if (type == QE_STRING) blank.dict = std::make_shared<DictData>();
        b->cols.push_back(blank);
        Column &c = b->cols.back();
        c.data = ctx->pool.alloc(column_bytes(type, nrows));
        if (nrows > 0) c.validity = (uint64_t *)ctx->pool.alloc(bitmap_bytes(nrows));
        return c;
    }

    // the converter's arguments for column k, with an empty patch list
    CsvConvArgs conv_args(int k, const Column &c) {
        QE_HIP(hipMemsetAsync(patch_count, 0, sizeof(u32), st));
        return CsvConvArgs{fields(k), c.data, (u64 *)c.validity, any_null + k, flags, patch_rows, patch_count, patch_cap};
    }

    // The fields rows[0..n) of a column (a device list) as the host reads them.  len: their unescaped lengths on the device and
    // a zero behind them, the scan's n + 1 elements; it holds the offsets afterwards.  Two copies come down: offsets, bytes.
    PackedFields pack_fields(const CsvFields &f, const i64 *rows, i64 count, i64 *len) {
        PackedFields p;
        scan(ctx, S, len, count);
        p.off = std::vector<i64>((size_t)count + 1);
        QE_HIP(hipMemcpyAsync(p.off.data(), len, sizeof(i64) * (count + 1), hipMemcpyDeviceToHost, st));
        QE_HIP(hipStreamSynchronize(st));
        const size_t total = (size_t)p.off[(size_t)count];
        unsigned char *packed = dev_array<unsigned char>(S, total);
        launch_csv_pack_fields(st, f, rows, count, len, packed);
        p.bytes.assign(total, '\0');
        if (total > 0) QE_HIP(hipMemcpyAsync(&p.bytes[0], packed, total, hipMemcpyDeviceToHost, st));
        QE_HIP(hipStreamSynchronize(st));
        return p;
    }

    // 4a: DOUBLE.  The fields that the device leaves undecided come down packed, in the order of patch_rows; the host's
    // converter decides them and one scatter through patch_rows puts the values in place.
    void double_column(int k, Column &c) {
        const CsvConvArgs a = conv_args(k, c);
        launch_csv_convert_double(st, a);
        const u32 np = read_back(ctx, patch_count);
        if (read_back(ctx, flags) & (QE_CSV_BAD_NUMBER | QE_CSV_PATCH_OVERFLOW)) throw FallBack{};
        if (np == 0) return;
        i64 *len = dev_array<i64>(S, (size_t)np + 1);
        QE_HIP(hipMemsetAsync(len + np, 0, sizeof(i64), st));
        launch_csv_field_len(st, a.f, patch_rows, np, len);
        const PackedFields p = pack_fields(a.f, patch_rows, np, len);
        std::vector<double> vals(np);
        for (u32 j = 0; j < np; j++)
            if (!java_parse_double(p.bytes.data() + p.off[j], (size_t)(p.off[j + 1] - p.off[j]), vals[j])) throw FallBack{};
        double *dvals = dev_array<double>(S, np);
        QE_HIP(hipMemcpyAsync(dvals, vals.data(), sizeof(double) * np, hipMemcpyHostToDevice, st));
        launch_csv_scatter_f64(st, (double *)c.data, patch_rows, dvals, np);
        QE_HIP(hipStreamSynchronize(st));
        ctx->csv_stats.host_patched_fields += np;
    }

    // 4a: BOOLEAN
    void boolean_column(int k, Column &c) { launch_csv_convert_bool(st, conv_args(k, c)); }

    // 4b: STRING.  Codes in order of first appearance, and the distinct strings as the column's dictionary
    void string_column(int k, Column &c) {
        u64 cap = 64;
        while (cap < (u64)nrows * 2) cap <<= 1;
        CsvDictArgs a{};
        a.f = fields(k);
        a.hash = dev_array<u64>(S, (size_t)nrows);
        a.slots = dev_array<u32>(S, cap);
        a.first = dev_array<u32>(S, cap);
        a.mask = cap - 1;
        a.row_slot = dev_array<u32>(S, (size_t)nrows);
        a.rank = dev_array<i64>(S, (size_t)nrows + 1);
        a.codes = (int *)c.data;
        a.validity = (u64 *)c.validity;
        a.any_null = any_null + k;
        QE_HIP(hipMemsetAsync(a.slots, 0xFF, cap * sizeof(u32), st));
        QE_HIP(hipMemsetAsync(a.first, 0xFF, cap * sizeof(u32), st));
        QE_HIP(hipMemsetAsync(a.rank + nrows, 0, sizeof(i64), st));
        launch_csv_dict_build(st, a);
        scan(ctx, S, a.rank, nrows);
        const i64 nd = read_back(ctx, a.rank + nrows);
        a.dist_row = dev_array<i64>(S, (size_t)nd);
        a.dist_len = dev_array<i64>(S, (size_t)nd + 1);
        QE_HIP(hipMemsetAsync(a.dist_len + nd, 0, sizeof(i64), st));
        launch_csv_dict_codes(st, a);
        PackedFields p = pack_fields(a.f, a.dist_row, nd, a.dist_len);
        DictData &d = *c.dict;
        d.entries.reserve((size_t)nd);
        for (i64 j = 0; j < nd; j++) {
            d.entries.emplace_back(p.bytes, (size_t)p.off[(size_t)j], (size_t)(p.off[(size_t)j + 1] - p.off[(size_t)j]));
            d.index.emplace(d.entries.back(), (int32_t)j);
        }
    }

    // a column without NULL carries no validity bitmap, like the host's any_null
    void drop_validity(qe_batch *b) {
        if (nrows == 0) return;
        std::vector<u32> nulls(b->cols.size());
        if (!nulls.empty()) QE_HIP(hipMemcpyAsync(nulls.data(), any_null, sizeof(u32) * nulls.size(), hipMemcpyDeviceToHost, st));
        QE_HIP(hipStreamSynchronize(st));
        for (size_t k = 0; k < nulls.size(); k++)
            if (!nulls[k]) {
                ctx->pool.release(b->cols[k].validity);
                b->cols[k].validity = nullptr;
            }
    }
};

// The device passes over the text in `dev` (n bytes, padded with zeros to whole tiles).  Throws FallBack.
qe_batch *parse_on_device(qe_ctx *ctx, PoolScratch &S, const unsigned char *dev, i64 n, const Request &rq, const std::vector<int> &idx) {
    Passes p(ctx, S, dev, n);
    p.field_spans(p.record_starts(), idx);
    std::unique_ptr<qe_batch, BatchDeleter> b(new qe_batch(), BatchDeleter{ctx});   // its columns go back to the pool unless it is released
    b->nrows = p.nrows;
    p.begin_columns(rq.nfields);
    for (int k = 0; k < rq.nfields; k++) {
        Column &c = p.add_column(b.get(), rq.types[k]);
        if (p.nrows == 0) continue;
        if (c.type == QE_DOUBLE) p.double_column(k, c);
        else if (c.type == QE_BOOLEAN) p.boolean_column(k, c);
        else p.string_column(k, c);
    }
    QE_HIP(hipGetLastError());
    p.drop_validity(b.get());
    QE_HIP(hipStreamSynchronize(ctx->stream));
    return b.release();
}

// What both entry points do: check, header, upload, the device passes or the host parser (host_parse: the table of the same
// input from qe_csv_parse / qe_csv_parse_file), and the stats of the call.  source_ok: the caller's own argument is usable
int32_t parse_source(qe_ctx *ctx, const Request &rq, qe_batch **out, bool source_ok, TextSource &src,
                     const std::function<int32_t(qe_csv_table **)> &host_parse) {
    if (!ctx || !out || rq.nfields < 0 || (rq.nfields > 0 && (!rq.names || !rq.types))) return QE_ERR_INVALID_ARG;
    *out = nullptr;
    ctx->csv_stats = qe_csv_device_stats{};
    if (ctx->device < 0) {
        ctx->last_error = "planning-only context (QE_DEVICE_NONE): qe_csv_parse_device needs a HIP device; libqe_hip has no CPU fallback";
        return QE_ERR_HIP;
    }
    if (!source_ok) return QE_ERR_INVALID_ARG;
    ctx->csv_stats.text_bytes = (int64_t)src.nbytes;   // of bytes in memory; a file's size is known once it is open
    bool fallback = false;
    int32_t st = guarded(ctx, [&] {
        QE_HIP(hipSetDevice(ctx->device));
        src.open();
        ctx->csv_stats.text_bytes = (int64_t)src.nbytes;
        const std::pair<const char *, size_t> head = src.head();
        size_t body = 0;
        std::vector<int> idx;
        if (!resolve_header(head.first, head.second, rq, body, idx) || (body == head.second && head.second < src.nbytes)) {
            fallback = true;
            return;
        }
        PoolScratch S(ctx);
        const size_t n = src.nbytes - body;
        auto t0 = Clock::now();
        unsigned char *dev = alloc_text(ctx, S, n);
        upload(ctx, src, body, dev, n);
        ctx->csv_stats.h2d_ms = ms_since(t0);
        t0 = Clock::now();
        try {
            *out = parse_on_device(ctx, S, dev, (i64)n, rq, idx);
        } catch (const FallBack &) {
            fallback = true;
            ctx->csv_stats.host_patched_fields = 0;
            return;
        }
        ctx->csv_stats.kernel_ms = ms_since(t0);
        ctx->csv_stats.nrows = (*out)->nrows;
    });
    if (st != QE_OK || !fallback) return st;
    ctx->csv_stats.host_fallback = 1;
    qe_csv_table *t = nullptr;
    st = host_parse(&t);
    if (st != QE_OK) return st;
    st = qe_csv_pin(ctx, t, out);
    if (st == QE_OK) ctx->csv_stats.nrows = qe_csv_nrows(t);
    qe_csv_free(ctx, t);
    return st;
}

}  // namespace
}  // namespace qe

using namespace qe;

extern "C" {

int32_t qe_csv_parse_device(qe_ctx *ctx, const char *data, size_t nbytes, int32_t nfields, const char *const *names,
                            const int32_t *types, qe_batch **out) {
    MemSource src(data, nbytes);
    return parse_source(ctx, Request{nfields, names, types}, out, data || !nbytes, src,
                        [&](qe_csv_table **t) { return qe_csv_parse(ctx, data, nbytes, nfields, names, types, t); });
}

int32_t qe_csv_parse_file_device(qe_ctx *ctx, const char *path, int32_t nfields, const char *const *names,
                                 const int32_t *types, qe_batch **out) {
    FileSource src(path);
    return parse_source(ctx, Request{nfields, names, types}, out, path != nullptr, src,
                        [&](qe_csv_table **t) { return qe_csv_parse_file(ctx, path, nfields, names, types, t); });
}

int32_t qe_csv_device_last_stats(const qe_ctx *ctx, qe_csv_device_stats *out) {
    if (!ctx || !out) return QE_ERR_INVALID_ARG;
    *out = ctx->csv_stats;
    return QE_OK;
}

}  // extern "C"
