/*
 * qe_hip.h -- C ABI of libqe_hip.so: the MI355X (gfx950) drop-in for the
 * Filter/Projection hot path of jhorstmann/queryengine.
 *
 * The reference has no native boundary of its own: its seam is
 * the Kotlin operator API.  Each entry point below names the reference
 * interface it sits beneath (paths relative to
 * /root/reference/src/main/java/net/jhorstmann/queryengine/); INTEGRATION.md
 * shows the Panama/JNI binding a maintainer would add on the Kotlin side.
 *
 * Conventions: plain C, no C++ types, no exceptions across the boundary.
 * Every call returns int32 status (QE_OK = 0); qe_last_error(ctx) gives the
 * message of the last failing call on that context.  The caller owns host
 * buffers it passes in; the library owns device memory and result objects
 * until the matching *_free.  One qe_ctx = one device + one HIP stream; a
 * context is NOT thread-safe, distinct contexts are independent (the
 * reference runs one thread per plan: operator/Operators.kt:5-32).
 */
#ifndef QE_HIP_H
#define QE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QE_ABI_VERSION 1

/* ---- status codes ---------------------------------------------------------- */
enum {
    QE_OK = 0,
    QE_ERR_INVALID_ARG = 1,   /* IllegalArgumentException analogue */
    QE_ERR_PROGRAM = 2,       /* malformed / ill-typed expression program (TypeCheckException analogue) */
    QE_ERR_HIP = 3,           /* HIP runtime / hiprtc failure, message carries the HIP error string */
    QE_ERR_OOM = 4,
    QE_ERR_UNSUPPORTED = 5,
    QE_ERR_INTERNAL = 6,      /* includes a look-back spin that hit its bound */
    QE_ERR_COMM = 7           /* RCCL failure */
};

/* ---- data types: data/Schema.kt:3-5 ordinals + extensions ------------------ */
enum {
    QE_STRING = 0,    /* int32 dictionary codes + qe_dict */
    QE_DOUBLE = 1,    /* f64 */
    QE_BOOLEAN = 2,   /* value bitmap: row i = word i>>6, bit i&63 (LSB first) */
    QE_INT64 = 3,     /* extension: Java long semantics */
    QE_INT32 = 4      /* extension: Java int semantics */
};

/* ---- expression program ----------------------------------------------------
 * An Expression tree (ast/Expressions.kt:6-62) is serialised in POSTFIX order
 * (operands first), little endian:
 *
 *   header : 'Q' 'E' 'X' <version=1>
 *   QE_OP_COLUMN       u8 op, u8 type, u16 index          ColumnExpression(name, index, dataType) :60-62
 *   QE_OP_NUM_LITERAL  u8 op, f64 value                   NumericLiteralExpression :17-21 (always DOUBLE)
 *   QE_OP_BOOL_LITERAL u8 op, u8 value                    BooleanLiteralExpression :23-27
 *   QE_OP_STR_LITERAL  u8 op, u16 nbytes, UTF-8 bytes     StringLiteralExpression :29-33
 *   QE_OP_LIST_LITERAL u8 op, u8 elem_type, u32 count,    extension: the literal list of IN.  elem_type is QE_DOUBLE,
 *                      count payloads                     QE_STRING or QE_BOOLEAN; a payload is an f64, or u16 nbytes +
 *                                                         UTF-8 bytes, or a u8.  Pushes ONE value (the whole list);
 *                                                         1 <= count <= 65536; only IN may consume it
 *   QE_OP_FUNCTION     u8 op, u8 function, u8 type        FunctionExpression :36-45; function = Function.ordinal
 *                                                         (ast/Functions.kt:7-22), type = dataTypeNullable or 0xFF
 *
 * qe_expr_compile is the analogue of compileExpression (evaluator/Compiler.kt:20-26)
 * plus the bytecode verifier pass (BytecodeCompiler.kt:138, MaxStackVisitor :177-196):
 * it checks stack discipline, arity and operand types and infers result types.
 */
enum { QE_OP_COLUMN = 1, QE_OP_NUM_LITERAL = 2, QE_OP_BOOL_LITERAL = 3, QE_OP_STR_LITERAL = 4, QE_OP_LIST_LITERAL = 5, QE_OP_FUNCTION = 16 };

/* Ordinals 0-16 are the reference's (ast/Functions.kt:7-22).  Ordinals 17-22, 24 and 25 are extensions the reference's
 * enum does not have (additive: header version and ABI version stay 1):
 *   IS_NULL / IS_NOT_NULL  1 operand of any type -> BOOLEAN, never NULL: the validity of the operand EXPRESSION
 *   COALESCE               2 operands typed like the branches of IF -> a where a is valid, else b (NULL iff both are)
 *   ABS                    numeric -> operand type; Math.abs (-0.0 -> 0.0, NaN stays NaN, MIN_VALUE stays MIN_VALUE)
 *   FLOOR / CEIL           numeric -> operand type; Math.floor / Math.ceil on DOUBLE, the identity on integers
 *   IN                     (value, list literal) -> BOOLEAN, NULL exactly where the value is.  By definition
 *                          value = L1 OR .. OR value = Lm under CMP_EQ on the promoted operands: the value and the list are
 *                          typed as the operands of CMP_EQ (an integer value is cast to DOUBLE, every numeric literal being
 *                          DOUBLE); DOUBLE compares as Double.equals (one NaN, -0.0 <> 0.0) in both cmp_semantics.  Duplicates
 *                          are allowed, an empty list is a program error, more than 65536 items are QE_ERR_UNSUPPORTED
 *                          (a larger set is a SEMI join).  NOT IN is NOT(IN(..)).
 *   LIKE                   (STRING value, STRING literal pattern) -> BOOLEAN, NULL exactly where the value is.  Whole-string,
 *                          case-sensitive match by code points (an invalid UTF-8 byte is its own unit): % matches zero or more,
 *                          _ exactly one, \ makes the next character literal (a trailing lone \ is a program error).
 * ABS, FLOOR and CEIL map NULL to NULL. */
enum {
    QE_FN_AND = 0, QE_FN_OR, QE_FN_IF, QE_FN_NOT, QE_FN_UNARY_MINUS, QE_FN_UNARY_PLUS, QE_FN_MUL, QE_FN_DIV,
    QE_FN_MOD, QE_FN_ADD, QE_FN_SUB, QE_FN_CMP_LT, QE_FN_CMP_LE, QE_FN_CMP_GE, QE_FN_CMP_GT, QE_FN_CMP_EQ,
    QE_FN_CMP_NE,
    QE_FN_IS_NULL = 17, QE_FN_IS_NOT_NULL, QE_FN_COALESCE, QE_FN_ABS, QE_FN_FLOOR, QE_FN_CEIL, /* 23 is not assigned: unknown */
    QE_FN_IN = 24, QE_FN_LIKE = 25, QE_FN_COUNT_
};

/* ast/Functions.kt:24-26 ordinals (ANY/ALL are TODO() in the reference: Accumulators.kt:16-17) */
enum { QE_AGG_MIN = 0, QE_AGG_MAX = 1, QE_AGG_SUM = 2, QE_AGG_COUNT = 3, QE_AGG_AVG = 4 };

/* ---- options ---------------------------------------------------------------- */
enum {
    QE_EXEC_FUSED = 0,     /* one single-pass fused kernel per plan, JIT-specialised with hiprtc
                              (the on-device analogue of Mode.BYTECODE_COMPILER / compileProjection,
                              BytecodeCompiler.kt:37-132) */
    QE_EXEC_PER_NODE = 1   /* one precompiled kernel per expression node, filter first
                              (the analogue of Mode.INTERPRETER's tree walk, Interpreter.kt:29-109) */
};
enum {
    QE_CMP_TOTAL_ORDER = 0, /* java.lang.Double.compare: INTERPRETER + BYTECODE_COMPILER */
    QE_CMP_IEEE = 1         /* primitive <,<=,>=,>: CLOSURE_COMPILER (ClosureCompiler.kt:127-130) */
};

typedef struct {
    uint32_t struct_size;        /* = sizeof(qe_options) */
    int32_t exec_mode;           /* QE_EXEC_* */
    int32_t cmp_semantics;       /* QE_CMP_* */
    int32_t profile;             /* 1: bracket the dominant kernel with HIP events (qe_ctx_kernel_time) */
    int64_t result_capacity_rows;/* 0 = size result buffers for the worst case (every row kept) */
    const char *jit_cache_dir;   /* NULL = $QE_JIT_CACHE_DIR or <library dir>/jit_cache */
    int32_t tuning[8];           /* kernel tuning knobs, 0 = default; see DESIGN.md */
} qe_options;

typedef struct qe_ctx qe_ctx;
typedef struct qe_dict qe_dict;
typedef struct qe_batch qe_batch;
typedef struct qe_expr qe_expr;
typedef struct qe_result qe_result;

/* ---- context ---------------------------------------------------------------- */
/* device = QE_DEVICE_NONE gives a PLANNING-ONLY context: expressions can be
 * compiled and verified, plans generated and JIT-compiled into the cache (hiprtc
 * needs no GPU), but every call that would touch device memory fails with
 * QE_ERR_HIP -- there is no CPU execution path in this library. */
#define QE_DEVICE_NONE (-1)
int32_t qe_abi_version(void);
/* last error of a failed qe_ctx_create (ctx == NULL) or of ctx */
const char *qe_last_error(const qe_ctx *ctx);
int32_t qe_ctx_create(int32_t device, const qe_options *opts, qe_ctx **out);
void qe_ctx_destroy(qe_ctx *ctx);
int32_t qe_ctx_set_exec_mode(qe_ctx *ctx, int32_t exec_mode);
int32_t qe_ctx_set_cmp_semantics(qe_ctx *ctx, int32_t cmp_semantics);
/* HIP-event time of the dominant kernel (needs opts.profile): last launch, sum and count since reset */
int32_t qe_ctx_kernel_time(qe_ctx *ctx, double *last_ms, double *total_ms, int64_t *launches);
int32_t qe_ctx_reset_kernel_time(qe_ctx *ctx);
int32_t qe_ctx_synchronize(qe_ctx *ctx);
/* release cached device buffers back to the driver */
int32_t qe_ctx_trim(qe_ctx *ctx);

/* ---- dictionaries (STRING columns) -------------------------------------------- */
int32_t qe_dict_create(qe_ctx *ctx, int32_t nentries, const char *const *utf8, qe_dict **out);
int32_t qe_dict_size(const qe_dict *dict);
const char *qe_dict_entry(const qe_dict *dict, int32_t code);
void qe_dict_free(qe_ctx *ctx, qe_dict *dict);

/* ---- batches: the columnar scan leaf --------------------------------------------
 * Replaces MemoryTable / MemorySourceOperator (data/MemoryTable.kt:7-19,
 * operator/MemorySourceOperator.kt:5-36) beneath Table.getScanOperator
 * (data/Table.kt:8): columns are copied to HBM ONCE and stay resident across
 * repeated open()/close() of the operator (T/SimpleSumBenchmark.java:63-94). */
typedef struct {
    int32_t type;              /* QE_* data type */
    int32_t reserved;
    const void *data;          /* nrows elements (BOOLEAN: ceil(nrows/64) uint64 words) */
    const uint64_t *validity;  /* ceil(nrows/64) words, bit = 1 valid; NULL = all valid */
    const qe_dict *dict;       /* QE_STRING only */
} qe_col_desc;

/* host buffers -> device (H2D once) */
int32_t qe_batch_create(qe_ctx *ctx, int64_t nrows, int32_t ncols, const qe_col_desc *cols, qe_batch **out);
/* data/validity already are device pointers owned by the caller (zero copy) */
int32_t qe_batch_wrap_device(qe_ctx *ctx, int64_t nrows, int32_t ncols, const qe_col_desc *cols, qe_batch **out);

/* schema only (types, nullability = validity != NULL, dictionaries; data ignored): for plan-time
 * preparation (qe_filter_project_prepare / _source) without device memory */
int32_t qe_batch_describe(qe_ctx *ctx, int64_t nrows, int32_t ncols, const qe_col_desc *cols, qe_batch **out);

/* synthetic columns generated on the device from the GLOBAL row index;
 * avoids a 24 GB H2D for the 1 B-row configurations and makes shards reproducible */
enum { QE_GEN_I64_MOD = 0, QE_GEN_I32_MOD = 1, QE_GEN_F64_UNIT = 2, QE_GEN_F64_MOD = 3, QE_GEN_F64_STEP = 4,
       QE_GEN_F64_PRICE = 5, QE_GEN_DICT_MOD = 6,
       QE_GEN_I64_ROWID = 7 /* value = global row index: order-preservation checks */ };
typedef struct {
    int32_t kind;
    int32_t col_id;       /* random stream id */
    uint64_t modulus;
    int64_t offset;
    double step;
    int32_t aux_col_id;
    int32_t null_pct;     /* 0 = no validity bitmap */
    const qe_dict *dict;  /* QE_GEN_DICT_MOD */
} qe_gen_spec;
int32_t qe_batch_generate(qe_ctx *ctx, uint64_t seed, int64_t row_begin, int64_t nrows, int32_t ncols,
                          const qe_gen_spec *specs, qe_batch **out);

int64_t qe_batch_nrows(const qe_batch *batch);
int32_t qe_batch_ncols(const qe_batch *batch);
int32_t qe_batch_column_type(const qe_batch *batch, int32_t col);
/* device -> host copy of rows [row_begin, row_begin + nrows); row_begin must be a multiple of 64.
 * validity_out may be NULL; if the column has no validity bitmap it is filled with ones */
int32_t qe_batch_column_to_host(qe_ctx *ctx, const qe_batch *batch, int32_t col, int64_t row_begin, int64_t nrows,
                                void *data_out, uint64_t *validity_out);
void qe_batch_free(qe_ctx *ctx, qe_batch *batch);

/* ---- CSV text -> columns ------------------------------------------------------------------
 * The on-disk step in front of the path: replaces the row-at-a-time CSV scan leaves CsvTable / CsvSourceOperator
 * (data/CsvTable.kt:12-29, operator/CsvSourceOperator.kt:52-76) and UnivocityCsvTable / UnivocityCsvScanOperator
 * (data/UnivocityCsvTable.kt:10-69) beneath Table.getScanOperator (data/Table.kt:8).  Same conversion rules (first
 * record = header, fields located by header name, empty lines skipped, missing or empty field = NULL, String.toBoolean,
 * String.toDouble = java.lang.Double.parseDouble; a malformed number is QE_ERR_INVALID_ARG with the reference's
 * NumberFormatException text), but the result is one contiguous array per projected field in the qe_col_desc layout
 * (+ validity bitmap, + a dictionary in order of first appearance for STRING) that qe_csv_pin copies to HBM once.
 * types[] may hold QE_STRING, QE_DOUBLE, QE_BOOLEAN (data/Schema.kt:3-5).  Host-side, needs no device. */
typedef struct qe_csv_table qe_csv_table;
int32_t qe_csv_parse(qe_ctx *ctx, const char *utf8, size_t nbytes, int32_t nfields, const char *const *names,
                     const int32_t *types, qe_csv_table **out);
int32_t qe_csv_parse_file(qe_ctx *ctx, const char *path, int32_t nfields, const char *const *names, const int32_t *types,
                          qe_csv_table **out);
int64_t qe_csv_nrows(const qe_csv_table *table);
int32_t qe_csv_ncols(const qe_csv_table *table);
/* host view of one parsed column (pointers owned by the table; validity == NULL: no NULL in the column) */
int32_t qe_csv_column(const qe_csv_table *table, int32_t col, qe_col_desc *out);
/* = qe_batch_create on the table's columns ("pin to HBM once"); the batch keeps the dictionaries alive */
int32_t qe_csv_pin(qe_ctx *ctx, const qe_csv_table *table, qe_batch **out);
void qe_csv_free(qe_ctx *ctx, qe_csv_table *table);

/* The same conversion with the parsing on the device: the header is resolved on the host, the text after it goes to HBM
 * once, and kernels find the records and fields and convert them straight into the batch's device columns (DESIGN.md
 * 3.6).  Same rules, same batch as qe_csv_parse + qe_csv_pin, or the same status and error text: wherever the device
 * cannot prove that it reads the text as the host parser does (a '"' that is not a field's enclosing quote, an
 * unterminated quote, a malformed number), the whole input goes through qe_csv_parse + qe_csv_pin instead.  The batch owns
 * its device columns and dictionaries.  A planning-only context fails with QE_ERR_HIP; a text larger than free device
 * memory with QE_ERR_OOM.  The file variant reads the file in chunks through pinned staging, the read of one chunk beside
 * the copy of the previous one. */
int32_t qe_csv_parse_device(qe_ctx *ctx, const char *utf8, size_t nbytes, int32_t nfields, const char *const *names,
                            const int32_t *types, qe_batch **out);
int32_t qe_csv_parse_file_device(qe_ctx *ctx, const char *path, int32_t nfields, const char *const *names,
                                 const int32_t *types, qe_batch **out);
/* what the last qe_csv_parse*_device call on this context did */
typedef struct {
    int64_t text_bytes;            /* bytes of the input */
    int64_t nrows;
    int64_t host_patched_fields;   /* DOUBLE fields the device left to the host converter (hexadecimal, > 19 digits) */
    int32_t host_fallback;         /* 1: the whole input went through qe_csv_parse + qe_csv_pin */
    int32_t reserved;
    double h2d_ms;                 /* wall time of the text's copy to the device (file variant: read + copy) */
    double kernel_ms;              /* wall time from the text on the device to the finished batch */
} qe_csv_device_stats;
int32_t qe_csv_device_last_stats(const qe_ctx *ctx, qe_csv_device_stats *out);
/* 1 if the batch's column carries a validity bitmap (the plan of a query over it is specialised on that), 0 if not, -1 on
 * a bad argument */
int32_t qe_batch_column_nullable(const qe_batch *batch, int32_t col);
/* a new handle on the dictionary of a STRING column (shared with the batch; free with qe_dict_free) */
int32_t qe_batch_column_dict(const qe_batch *batch, int32_t col, qe_dict **out);

/* ---- expressions ------------------------------------------------------------------ */
/* compileExpression(expression, mode): evaluator/Compiler.kt:20-26 */
int32_t qe_expr_compile(qe_ctx *ctx, const uint8_t *program, size_t len, qe_expr **out);
int32_t qe_expr_result_type(const qe_expr *expr);
void qe_expr_free(qe_ctx *ctx, qe_expr *expr);

/* ---- the hot path ------------------------------------------------------------------
 * Projection(Filter(Scan)) in one call: FilterOperator.next (operator/FilterOperator.kt:14-25)
 * + ProjectionOperator.next (operator/ProjectionOperator.kt:15-19) /
 * CompiledProjectionOperator (BytecodeCompiler.kt:37-132) for every row of the
 * batch, order preserving.  filter may be NULL (no Filter node).  The analogue of
 * the Filter/Projection branches of buildPhysicalPlan (evaluator/Planner.kt:33-46). */
int32_t qe_filter_project(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                          const qe_expr *const *projections, int32_t nproj, qe_result **out);
/* plan-time preparation only (JIT compile + cache), no execution: what buildPhysicalPlan does */
int32_t qe_filter_project_prepare(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                  const qe_expr *const *projections, int32_t nproj);

/* GlobalAggregation(Projection(Filter(Scan))):
 * GlobalAggregationOperator.open (operator/GlobalAggregationOperator.kt:10-25) with
 * Accumulators.kt:26-107 semantics: nulls skipped, empty => null, COUNT => count.
 * SUM/AVG use a fixed-shape tree reduction (deterministic: repeated executions, also on a
 * fresh context, give the same bits; not the reference's sequential order: within
 * gamma_c * sum|x| of the exact sum, see DESIGN.md 3.2 and tests/test_gpu_aggregate_numerics.py). */
int32_t qe_filter_aggregate(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                            const qe_expr *const *exprs, const int32_t *agg_fns, int32_t nagg,
                            double *out_values, uint8_t *out_valid, int64_t *out_selected_rows);

/* GroupByAggregation(Projection(Filter(Scan))): GroupByAggregationOperator.open
 * (operator/GroupByAggregationOperator.kt:21-49).  The result has nkeys key columns followed by nagg DOUBLE
 * aggregate columns (NULL for an empty MIN/MAX/SUM/AVG, COUNT as a double), one row per group, in INSERTION
 * order of the groups (LinkedHashMap, :22; pinned by T/evaluator/QueryTest.kt:25-30); NULL is a key value.
 * Keys are expressions of any type -- the reference groups on the boxed key tuple (:33-37; Tripdata.kt:27-31 groups by a
 * DOUBLE column): STRING (dictionary) / BOOLEAN keys with at most 2^20 combinations index a dense table; DOUBLE / INT64 /
 * INT32 keys (Double.equals: all NaNs one group, -0.0 and 0.0 two) and larger combinations are hashed.
 * SUM/AVG use native f64 atomics: exact when every partial sum is representable, otherwise order dependent in the last
 * bits: within gamma_c * sum|x| of the EXACT sum of a group's c valid values, gamma_c = c*u / (1 - c*u), u = 2^-53 (the
 * bound of c terms added in any order; AVG: gamma_(c+1) * sum|x| / c, plus 2^-1075 for a quotient in the subnormal range),
 * on every accumulation route -- pinned against math.fsum by tests/test_gpu_aggregate_numerics.py.  Decided special values: a group holding a NaN, or both infinities,
 * sums to NaN; one infinity, to that infinity; only -0.0, to +0.0 (Accumulators.kt:40 starts from 0.0) while its MIN and
 * MAX are -0.0; MIN/MAX let NaN win and order -0.0 below +0.0; all values NULL => NULL, COUNT 0.  Subnormal values are
 * kept by the LDS and L2 f64 atomic adds (sums of multiples of 2^-1074 come out bit-exact). */
int32_t qe_filter_groupby(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                          const qe_expr *const *keys, int32_t nkeys,
                          const qe_expr *const *exprs, const int32_t *agg_fns, int32_t nagg, qe_result **out);

int32_t qe_filter_groupby_prepare(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                  const qe_expr *const *keys, int32_t nkeys,
                                  const qe_expr *const *exprs, const int32_t *agg_fns, int32_t nagg);

/* what the last qe_filter_groupby of this context did (zeros before the first one): qe_ctx_last_form tells
 * the three forms apart, this the routes inside them and what the call had to repeat.
 * out[0] the route that produced the result, QE_GROUPBY_ROUTE_*;
 * out[1] launches of this call that were abandoned and repeated another way: the error word came back non-zero (3: a global
 *        or id table more than half full or a probe sequence exhausted, 4: the keys do not fit a workgroup's LDS table,
 *        6: a hash partition's table filled up) or the skew rule of the hash-partitioned form fired;
 * out[2] the capacity that sufficed: entries of the global table (HASHED), entries of the id table (DENSE_IDS), buckets per
 *        partition (HASH_PARTITIONED_*), groups per partition (DENSE_KEY_RANGE), groups of the table (DENSE_LDS, DENSE_GLOBAL);
 * out[3] partitions of the partitioned passes that ran (DENSE_IDS: of the dense pass over the ids), 0 where none did. */
enum { QE_GROUPBY_ROUTE_NONE = 0, QE_GROUPBY_ROUTE_DENSE_LDS = 1, QE_GROUPBY_ROUTE_DENSE_KEY_RANGE = 2,
       QE_GROUPBY_ROUTE_DENSE_GLOBAL = 3, QE_GROUPBY_ROUTE_HASHED = 4, QE_GROUPBY_ROUTE_DENSE_IDS = 5,
       QE_GROUPBY_ROUTE_HASH_PARTITIONED_HOST = 6, QE_GROUPBY_ROUTE_HASH_PARTITIONED_DEVICE = 7 };
int32_t qe_ctx_last_groupby_stats(const qe_ctx *ctx, int64_t out[4]);

/* plan-time preparation of the aggregate plan (JIT compile + cache), no execution */
int32_t qe_filter_aggregate_prepare(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                    const qe_expr *const *exprs, const int32_t *agg_fns, int32_t nagg);

/* ---- results --------------------------------------------------------------------------- */
typedef struct {
    int32_t type;
    int32_t nullable;
    const void *data;          /* DEVICE pointer: count elements (BOOLEAN: bitmap words) */
    const uint64_t *validity;  /* DEVICE pointer or NULL */
    int64_t count;
    const qe_dict *dict;       /* QE_STRING: dictionary of the output codes (owned by the result) */
} qe_col_view;

int64_t qe_result_count(const qe_result *result);
int32_t qe_result_ncols(const qe_result *result);
int32_t qe_result_column(const qe_result *result, int32_t col, qe_col_view *out);
/* copy one output column to the CALLER's host buffers sized for qe_result_count rows (pageable memory is fine: the bytes
 * are staged through pinned chunks and copied out by a few host threads while the next chunk is on the link) */
int32_t qe_result_column_to_host(qe_ctx *ctx, const qe_result *result, int32_t col, void *data_out,
                                 uint64_t *validity_out);
void qe_result_free(qe_ctx *ctx, qe_result *result);

/* Result -> host, the way a caller that materialises rows wants it (Main.kt:18 `physicalPlan.map { it }`;
 * operator/Operators.kt:5-11 hands out host rows): every column is copied into PINNED host memory owned by the library
 * (pooled per context: a re-opened operator does not pin again) on the context's COPY stream.  qe_result_to_host only
 * starts the copies and returns -- the next qe_filter_project (compute stream) runs beside them; qe_host_result_wait blocks
 * until the bytes are there; qe_host_result_column then gives HOST pointers in the qe_col_view (same layouts as on the
 * device; validity NULL = no NULL in the column); qe_host_result_free returns the buffers to the pool.  `result` must stay
 * alive until the wait has returned (qe_result_free waits for a copy that still reads it).  Into pinned memory the link
 * runs at its own rate (0.8 GB: ~15 ms) where a copy into pageable memory (qe_result_column_to_host) is bound by host
 * memcpy; the kernel itself is not overlapped with the copy of ITS OWN result: it takes 3 ms, the copy 15. */
typedef struct qe_host_result qe_host_result;
int32_t qe_result_to_host(qe_ctx *ctx, const qe_result *result, qe_host_result **out);
int32_t qe_host_result_wait(qe_ctx *ctx, qe_host_result *host);
int64_t qe_host_result_count(const qe_host_result *host);
int32_t qe_host_result_ncols(const qe_host_result *host);
int32_t qe_host_result_column(const qe_host_result *host, int32_t col, qe_col_view *out);
void qe_host_result_free(qe_ctx *ctx, qe_host_result *host);
/* Concatenate results of ONE device, in the given order, into a new result (value columns at row offsets, bitmap
 * columns shifted into place as 64-row words): what a host does that feeds a table batch by batch and still hands the
 * reference's single Operator (operator/Operators.kt:5-11) the whole result.  Parts must share schema and dictionaries. */
int32_t qe_result_concat(qe_ctx *ctx, const qe_result *const *parts, int32_t nparts, qe_result **out);

/* ORDER BY <column> of a materialised result, on the device: OrderByOperator.open (operator/OrderByOperator.kt:9-15) sorts
 * the rows STABLY with Kotlin's compareValues -- NULL first, Double.compareTo (-0.0 < 0.0, NaN greatest), String.compareTo
 * (UTF-16 code units), false < true.  `column` is 0-based (the planner's ORDER BY <ordinal> is 1-based: Planner.kt:60). */
int32_t qe_result_order_by(qe_ctx *ctx, const qe_result *result, int32_t column, qe_result **out);
/* ORDER BY key[0], key[1], .. [LIMIT k]: the rows of `result` under the comparator key[0], then key[1], .., sorted STABLY
 * (rows equal on every key keep their input order, in both directions).  An ascending key is the order above; a descending
 * key is the reversed comparator (compareValues(b, a), what compareByDescending / thenByDescending use): NaN first, 0.0
 * before -0.0, true before false, NULL LAST.  1 <= nkeys <= 8; a column may appear twice.  limit = k >= 0 returns exactly
 * the first min(k, n) rows of that order (k = 0: an empty result with the schema of the input); limit < 0: every row.
 * For 0 < k <= n / 2 the k-th smallest image of the first key is SELECTED on the device (8-bit radix select, the images are
 * only read) and just the rows up to it, ties included, are sorted and gathered; when those are more than half of the rows
 * (a boolean or few-valued first key) the full sort runs and is truncated -- the rows are the same either way.
 * One ascending key without a limit returns the same bytes as qe_result_order_by.  The reference has one ascending key
 * and no LIMIT (Query.g4:19); this is the Kotlin standard library's compareBy().thenByDescending() on a stable sortWith.
 * QE_ERR_INVALID_ARG: null pointer, nkeys or a column out of range, a STRING key without dictionary; *out = NULL on error. */
typedef struct { int32_t column; int32_t descending; } qe_sort_key;   /* column 0-based */
int32_t qe_result_order_by_keys(qe_ctx *ctx, const qe_result *result, const qe_sort_key *keys, int32_t nkeys, int64_t limit,
                                qe_result **out);
/* what the last qe_result_order_by_keys (or qe_result_order_by: one ascending key, no limit) of this context did:
 * out[0] path (0 full sort, 1 top-k selection), out[1] rows that went into the sort, out[2] radix passes run,
 * out[3] selection passes run */
int32_t qe_ctx_last_sort_stats(const qe_ctx *ctx, int64_t out[4]);

/* ---- hash equi-join of two device-resident sides ---------------------------------------------------------
 * The reference has no join (Query.g4 reads one table); this is the fact-to-dimension step that follows its operators.
 * A side is a result or a batch.  qe_join_build reads the build side's key columns once and keeps a table: the rows
 * whose key holds no NULL, sorted stably by the top bits of a 64-bit hash of the key, and a directory over those bits.
 * qe_join_probe joins a probe side against it and returns an ordinary result.
 *
 * Keys: 1 <= nkeys <= 4; key column i of the probe side pairs with key column i of the build side, and the two must have
 * the same type (any of the five).  Equality is the engine's `=`: Double.equals for DOUBLE, so every NaN is
 * one value and -0.0 != 0.0.  STRING keys compare by string, not by code: the sides may carry different dictionaries, and a
 * probe string the build dictionary does not hold matches nothing.  A row with a NULL in ANY key column matches nothing,
 * on either side.  A shared hash is never taken for a match: every key image is compared.
 *
 * Rows and order: that of a nested loop with the probe side outside, deterministic -- the same inputs give the same bytes
 * on every run and every context; nothing depends on the order in which atomics arrive.
 *   QE_JOIN_INNER  one row per (probe row, matching build row), in probe-row order and inside one probe row in build-row order
 *   QE_JOIN_LEFT   the same, plus one row for every probe row without a match, in its place, every build column NULL
 *   QE_JOIN_SEMI   every probe row with at least one match, once, in probe order
 *   QE_JOIN_ANTI   every probe row without a match (a NULL key is no match), in probe order
 *   QE_JOIN_RIGHT  a HEAD, exactly the rows of QE_JOIN_INNER in their order, then a TAIL: every build row that no probe row of
 *                  THIS call matched, once, in ascending build row index, every probe column of it NULL (validity 0, value
 *                  zero).  A build row with a NULL in a key matches nothing, so it is always in the tail
 *   QE_JOIN_FULL   the same with the rows of QE_JOIN_LEFT as the head
 * SEMI and ANTI take no build columns (nbuild_out == 0).  Zero rows on either side is an ordinary input: without probe rows
 * the tail is the whole build side; without build rows RIGHT is empty and FULL is LEFT.
 * The table is not changed by a probe: the marks of the matched build rows belong to the call (a bitmap over build rows in its
 * scratch), so a table may be probed FULL by one side and then with any type by another.  The marks are set by integer ORs
 * and read only after the pass that sets them; no atomic decides a position in the output.
 *
 * Columns: the listed probe columns, then the listed build columns; a column may be listed twice, a list may be empty,
 * but there must be at least one output column.  A STRING column carries its source's dictionary; nullability is that of
 * the source, and under LEFT every build column is nullable (an unmatched row: validity 0, value zero); under RIGHT every
 * probe column is nullable and the build columns are as the source, under FULL every column is nullable -- the schema follows
 * from the inputs' schemas and the join type alone.  RIGHT / FULL with no probe columns is legal.  The result has
 * the layouts of every other result: qe_result_order_by_keys, qe_result_to_host, qe_result_concat, qe_gather take it.
 *
 * Lifetime: the table reads the build side's columns again at probe time, so the build input must outlive the table; the
 * table keeps the dictionaries alive and may be probed any number of times.
 *
 * Errors (*out = NULL): QE_ERR_INVALID_ARG for a null pointer, both or neither member of a qe_join_input set, a column out
 * of range, paired key columns of different types, nkeys outside 1..4, a schema-only batch, an unknown join type, no
 * output column, build columns with SEMI / ANTI; QE_ERR_UNSUPPORTED for a side of more than 2^32 - 2 rows (rows are
 * uint32 with one sentinel, as in the sort); QE_ERR_HIP on a planning-only context; QE_ERR_OOM when the output does not
 * fit.  Output counts and offsets are 64-bit throughout (head + tail), and the tail's length is read back together with the
 * head's: one read-back per call.  The values 4 to 7 of the join type are unassigned and rejected.
 * Known limit: the matches of ONE probe row are walked by one lane, so a probe key with very many matches is slow. */
enum { QE_JOIN_INNER = 0, QE_JOIN_LEFT = 1, QE_JOIN_SEMI = 2, QE_JOIN_ANTI = 3, QE_JOIN_RIGHT = 8, QE_JOIN_FULL = 9 };
/* one side of a join: exactly one of the two is non-NULL */
typedef struct { const qe_result *result; const qe_batch *batch; } qe_join_input;
typedef struct qe_join_table qe_join_table;

int32_t qe_join_build(qe_ctx *ctx, const qe_join_input *build, const int32_t *key_cols, int32_t nkeys,
                      qe_join_table **out);
int64_t qe_join_table_rows(const qe_join_table *table);      /* build rows whose key holds no NULL */
void    qe_join_table_free(qe_ctx *ctx, qe_join_table *table);
int32_t qe_join_probe(qe_ctx *ctx, const qe_join_table *table, const qe_join_input *probe,
                      const int32_t *key_cols, int32_t nkeys, int32_t join_type,
                      const int32_t *probe_out_cols, int32_t nprobe_out,
                      const int32_t *build_out_cols, int32_t nbuild_out, qe_result **out);
/* what the last qe_join_build / qe_join_probe of this context did: out[0] build rows in the table, out[1] probe rows,
 * out[2] output rows (RIGHT / FULL: head + tail), out[3] longest candidate run one probe row scanned */
int32_t qe_ctx_last_join_stats(const qe_ctx *ctx, int64_t out[4]);
/* the last RIGHT or FULL call of this context (zeros before the first; other join types leave it alone):
 * out[0] 1 = qe_join_probe, 2 = qe_result_range_join; out[1] head rows; out[2] tail rows;
 * out[3] build / right rows matched at least once.  out[2] + out[3] = rows of the build / right side. */
int32_t qe_ctx_last_outer_stats(const qe_ctx *ctx, int64_t out[4]);

/* ---- window functions over a result -------------------------------------------------------------------------
 * The reference has no windows (Query.g4); this is the step that answers a question about a row relative to its neighbours
 * -- a running total per account, the rank of a row inside its group, the previous value of a series -- without copying the
 * sorted result to the host.  qe_result_window sorts `result` and appends one column per entry of `fns`.
 *
 * Rows and order: the output holds every input row, sorted STABLY by the partition columns ascending, then by `order`, under
 * the comparator of qe_result_order_by_keys (NULL first ascending, NULL last descending).  npart == 0: the whole input is one
 * partition; norder == 0: rows keep their input order inside a partition.  Two adjacent rows share a partition when that
 * comparator returns 0 on every partition column: NULL is a key value, all NaNs are one value, -0.0 != 0.0, STRING compares
 * by string -- the rule of the group-by keys.  PEERS are rows of one partition that compare 0 on every order key.
 *
 * Columns: all input columns first, types, nullability and dictionaries unchanged; then one column per entry of `fns`.
 *
 * Frame: qe_result_window always uses ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW within the partition.  It counts rows,
 * so peers are not pulled in.  Sliding and whole-partition frames: qe_result_window_frames below.
 *
 * Functions:
 *   ROW_NUMBER (1-based), RANK (row number of the first peer), DENSE_RANK: INT64, not nullable; `column` is ignored.
 *   SUM, MIN, MAX, AVG over a DOUBLE / INT64 / INT32 column: values are converted to double as the group-by aggregates
 *     convert them; DOUBLE, nullable; NULL inputs are skipped; the value is NULL until the partition has shown its first valid
 *     value (Accumulators.kt: empty => null).
 *   COUNT over a column of any type: the valid values so far; DOUBLE, not nullable, like group-by's COUNT.
 *   Special values follow the rules decided at qe_filter_groupby: a prefix holding a NaN, or both infinities, sums to NaN from
 *     that row to the partition's end; a prefix of only -0.0 sums to +0.0; MIN / MAX let NaN win and order -0.0 below +0.0.
 *   LAG / LEAD with 0 <= offset < 2^31 over a column of any type: value and validity of the row `offset` places before /
 *     after in the same partition; a row beyond the partition's edge gives NULL (validity 0, value zero); always nullable; a
 *     STRING output carries the source dictionary; offset 0 is the row itself.
 *
 * Determinism: the same inputs give the same bytes on every run and on every context.  Every running aggregate is a
 * fixed-shape scan -- per-tile reduce, one workgroup over the tile aggregates, per-tile downsweep -- in which the values that
 * are combined depend on the row count and the partition starts alone: no look-back, no result byte depends on the order in
 * which atomics arrive.
 *
 * Numerics: SUM is within gamma_c * sum|x| of the exact prefix sum, c = valid values in the prefix, gamma_c = c*u / (1 - c*u),
 * u = 2^-53 (the any-order bound stated at qe_filter_groupby); AVG follows the group-by's AVG bound (gamma_(c+1) * sum|x| / c);
 * integer-valued data below 2^53 comes out exact.
 *
 * Errors (*out = NULL): QE_ERR_INVALID_ARG for a null pointer, npart or norder negative, npart + norder > 8, nfn outside
 * 1..16, a column out of range, an unknown fn, SUM / MIN / MAX / AVG over BOOLEAN or STRING, a negative or too large offset, a
 * STRING key without a dictionary; QE_ERR_UNSUPPORTED for 2^32 rows or more, as in the sort; QE_ERR_HIP on a planning-only
 * context; QE_ERR_OOM when the output or the scratch does not fit.  Zero input rows give a zero-row result with the full
 * output schema. */
enum { QE_WIN_ROW_NUMBER = 0, QE_WIN_RANK, QE_WIN_DENSE_RANK,
       QE_WIN_SUM, QE_WIN_COUNT, QE_WIN_MIN, QE_WIN_MAX, QE_WIN_AVG,
       QE_WIN_LAG, QE_WIN_LEAD };
typedef struct { int32_t fn; int32_t column; int64_t offset; } qe_window_fn;  /* column: argument (ignored by the three ranks); offset: LAG/LEAD only */
int32_t qe_result_window(qe_ctx *ctx, const qe_result *result,
                         const int32_t *partition_cols, int32_t npart,
                         const qe_sort_key *order, int32_t norder,
                         const qe_window_fn *fns, int32_t nfn, qe_result **out);
/* ---- window frames --------------------------------------------------------------------------------------------------------
 * qe_result_window with a frame per function: ROWS BETWEEN `preceding` PRECEDING AND `following` FOLLOWING, each either
 * QE_FRAME_UNBOUNDED or a row count in [0, 2^31).  With the partition of row j being rows [start, end] of the sorted order,
 * the frame of row j is [lo, hi]:
 *     lo = start if preceding == QE_FRAME_UNBOUNDED, else max(start, j - preceding)
 *     hi = end   if following == QE_FRAME_UNBOUNDED, else min(end,   j + following)
 * so it always holds the current row and is never empty; it counts rows (ROWS mode): peers are not pulled in.  A moving
 * average is (p, f); a whole-partition value on every row is (UNBOUNDED, UNBOUNDED); (UNBOUNDED, 0) is the running frame,
 * and every function of qe_result_window given that frame here returns the bytes qe_result_window returns (qe_result_window
 * IS this call with that frame).  Rows, order, input columns, limits and errors are those of qe_result_window.
 *
 * Functions that read the frame:
 *   SUM, COUNT, MIN, MAX, AVG over the frame's rows: NULL handling, special values, the conversion to double and the output
 *     types are those of qe_result_window (DOUBLE; COUNT not nullable, the others NULL while the frame holds no valid value).
 *     A special value counts only while it is inside the frame: the rows after an Inf or a NaN has left are finite again.
 *   FIRST_VALUE, LAST_VALUE over a column of any type: value and validity of row lo / row hi; a NULL there is returned as
 *     NULL (no IGNORE NULLS); the output has the source column's type, nullability and dictionary.
 * Functions that ignore the frame: the three ranks and LAG / LEAD; preceding and following must both be 0 for them.
 *
 * How: a frame's value is only ever built from values of rows inside the frame, never as a difference of two running sums.
 * With W = preceding + following + 1, a forward scan P restarted at partition starts and at every row j with j % W == 0 and a
 * reverse scan S restarted at partition ends and after every row with j % W == W - 1 are kept; the frame touches at most two
 * adjacent blocks of W rows and its value is P[hi], S[lo] or combine(S[lo], P[hi]).  One-sided frames read one plain scan
 * (forward at hi, or reverse at lo).  The scans have the fixed shape described above, so the determinism statement holds for
 * frames: the same inputs give the same bytes on every run and every context, no look-back, no atomic feeds a result byte.
 *
 * Numerics: a framed SUM is within gamma_c * sum|x| of the exact sum of the frame's valid values, c = valid values IN THE FRAME
 * and sum|x| over the frame (not the prefix); AVG: gamma_(c+1) * sum|x| / c; integer-valued data below 2^53 comes out exact.
 *
 * Errors beyond those of qe_result_window (QE_ERR_INVALID_ARG, *out = NULL): preceding or following below -1 or >= 2^31; a
 * non-zero preceding or following on a rank or on LAG / LEAD; FIRST_VALUE / LAST_VALUE with a column out of range.
 * qe_ctx_last_window_stats reports this call too. */
#define QE_FRAME_UNBOUNDED (-1)
enum { QE_WIN_FIRST_VALUE = 10, QE_WIN_LAST_VALUE = 11 };   /* continue QE_WIN_*; known to qe_result_window_frames only */
typedef struct { int32_t fn; int32_t column; int64_t offset;   /* as qe_window_fn */
                 int64_t preceding; int64_t following; } qe_window_frame_fn;
int32_t qe_result_window_frames(qe_ctx *ctx, const qe_result *result,
                                const int32_t *partition_cols, int32_t npart,
                                const qe_sort_key *order, int32_t norder,
                                const qe_window_frame_fn *fns, int32_t nfn, qe_result **out);
/* what the last qe_result_window / qe_result_window_frames of this context did: out[0] rows, out[1] partitions, out[2] scan tiles (2048 rows each),
 * out[3] trips of the tile-aggregate scan (1024 tiles each) */
int32_t qe_ctx_last_window_stats(const qe_ctx *ctx, int64_t out[4]);

/* ---- ordered-set aggregates per group ------------------------------------------------------------------------
 * The aggregates that cannot be merged from partials -- a median or percentile, COUNT(DISTINCT x), the most frequent value --
 * per group, over a result, without copying sorted rows to the host.  The reference has none of them (Query.g4).  With no
 * function the call is SELECT DISTINCT over the group columns.
 *
 * Rows and order: one row per group, the groups ASCENDING by the group columns under the comparator of
 * qe_result_order_by_keys (NULL first, Double.compareTo, strings by compareTo, false < true).  This is NOT the insertion order
 * of qe_filter_groupby.  Two rows share a group exactly when two window rows share a partition: NULL is a key value, every NaN
 * is one value, -0.0 != 0.0, STRING compares by string.  ngroup == 0: the whole input is one group.
 *
 * Columns: the ngroup group columns first (type, dictionary and nullability of the source column), then one column per entry
 * of `fns`.  nfn == 0 is allowed when ngroup >= 1 and returns the distinct key tuples.
 * Limits: 0 <= ngroup <= 7 (group columns plus one argument are the sort's 8 keys), 0 <= nfn <= 16, ngroup + nfn >= 1.
 *
 * Functions.  The values of a group for column x are its non-NULL values v[0 .. c-1], ascending under the sort comparator
 * (Double.compareTo: -0.0 < 0.0, NaN greatest; false < true; strings by compareTo).
 *   COUNT_DISTINCT   any type.  The number of distinct v under the engine's `=`: all NaNs are one value, -0.0 and 0.0 are two.
 *                    DOUBLE, not nullable, like every COUNT here; 0 for a group without a valid value.
 *   PERCENTILE_DISC  any type, BOOLEAN and STRING included.  v[k], k = max(ceil(fraction * (double)c) - 1, 0), the product one
 *                    IEEE f64 multiplication.  Source type and dictionary, always nullable, NULL when c == 0.
 *   PERCENTILE_CONT  DOUBLE, INT64 or INT32.  The values are converted to double, as the group-by aggregates convert them,
 *                    AFTER sorting in the column's own order.  With h = fraction * (double)(c - 1), lo = floor(h), hi = ceil(h),
 *                    frac = h - lo: the value is v[lo] when frac == 0 or v[lo] and v[hi] have the same bits (as doubles), else
 *                    v[lo] + (v[hi] - v[lo]) * frac, evaluated in exactly this order without FMA contraction:
 *                    the result is defined to the bit.  The median of two equal infinities is that infinity; -Inf against
 *                    +Inf, or a NaN in reach, gives what the formula gives.  DOUBLE, always nullable, NULL when c == 0.
 *                    MEDIAN is PERCENTILE_CONT with fraction 0.5.
 *   MODE             any type.  The value of the longest run of equal values (equal under `=`); of several longest runs the
 *                    smallest value.  Source type and dictionary, always nullable, NULL when c == 0.
 * `fraction` is read by the two percentiles only.  A NULL output has validity 0 and value zero.
 *
 * Zero input rows: with ngroup >= 1 a zero-row result with the full schema; with ngroup == 0 one row, COUNT_DISTINCT 0 and
 * every other function NULL (Accumulators.kt: empty => null, as in qe_filter_aggregate).
 *
 * How: one stable sort by (group columns, argument) per DISTINCT argument column -- functions that share an argument share
 * the sort -- then the boundary flags of the window operator, ranks and compaction of those bitmaps, and one small pass per
 * function; columns that hold source values are gathered from the source through a per-group row list.
 *
 * Determinism: the same inputs give the same bytes on every run and every context.  No floating-point value is combined by an
 * atomic; the only atomics are an integer add (the group count) and an integer max (MODE), whose results do not depend on the
 * order of arrival.
 *
 * Errors (*out = NULL): QE_ERR_INVALID_ARG for a null pointer, ngroup or nfn out of range or both zero, a column out of range,
 * an unknown fn, PERCENTILE_CONT over BOOLEAN or STRING, a percentile fraction that is NaN or outside [0, 1], a STRING group or
 * argument column without a dictionary; QE_ERR_UNSUPPORTED for 2^32 rows or more; QE_ERR_HIP on a planning-only context;
 * QE_ERR_OOM when scratch or output does not fit. */
enum { QE_OSA_COUNT_DISTINCT = 0, QE_OSA_PERCENTILE_CONT = 1, QE_OSA_PERCENTILE_DISC = 2, QE_OSA_MODE = 3 };
typedef struct { int32_t fn; int32_t column; double fraction; } qe_ordered_agg;   /* fraction: the two percentiles only */
int32_t qe_result_group_ordered(qe_ctx *ctx, const qe_result *result,
                                const int32_t *group_cols, int32_t ngroup,
                                const qe_ordered_agg *fns, int32_t nfn, qe_result **out);
/* what the last qe_result_group_ordered of this context did: out[0] input rows, out[1] groups, out[2] sorts run, out[3] radix
 * passes of those sorts */
int32_t qe_ctx_last_ordered_stats(const qe_ctx *ctx, int64_t out[4]);

/* ---- set operations over two results ---------------------------------------------------------------------------
 * UNION, INTERSECT and EXCEPT of two results, each with its ALL form, without copying either to the host.  The reference has
 * none of them (Query.g4 reads one table).  A SEMI / ANTI join comes close to INTERSECT / EXCEPT but stops at four key columns,
 * never matches a NULL, keeps duplicates and cannot express the multiset forms.
 *
 * Schema: both sides have the same number of columns (at least one) and column i has the same type on both sides; all five
 * types are allowed and nothing is promoted.  An output column is nullable exactly when the column is nullable on either side,
 * for every op, so the output schema follows from the inputs' schemas alone.  `left` and `right` may be the same handle.
 *
 * Equality of two rows is the rule by which two rows share a group in qe_result_group_ordered, on every column: NULL is a
 * value and equals NULL, every NaN is one value, -0.0 is not 0.0, STRING compares by string, never by code.
 *
 * Dictionaries of STRING columns: if both sides carry the same dictionary object the output carries it too and no code
 * changes.  Otherwise the output carries a merged dictionary: the left dictionary's entries first, in their order, so left
 * codes are unchanged; after them the right dictionary's entries that the left does not hold, in the right dictionary's order
 * (an entry the right dictionary lists twice is appended twice and both codes stay apart).  Right codes are translated on the
 * device; a right entry that the left holds maps to the code the left dictionary finds for it (its first, if the left lists
 * the string twice).  A right code outside its dictionary becomes 0.
 *
 * Rows kept.  For a tuple that occurs cL times on the left and cR times on the right:
 *                   all == 0                            all == 1
 *   QE_SET_UNION      1                                   cL + cR
 *   QE_SET_INTERSECT  1 if cL > 0 and cR > 0, else 0      min(cL, cR)
 *   QE_SET_EXCEPT     1 if cL > 0 and cR == 0, else 0     max(cL - cR, 0)
 *
 * Order: UNION ALL returns the left rows in their order, then the right rows in theirs, and runs no sort.  Every other form
 * returns its rows ASCENDING by column 0, then column 1, and so on, under the comparator of qe_result_order_by_keys (NULL
 * first): the order of qe_result_group_ordered.  The k copies of a tuple are its first k rows in the sequence "left rows in
 * input order, then right rows in input order"; that fixes which NaN payload, and which of two codes of a twice-listed string,
 * comes out, and a kept row is a left row whenever the tuple occurs on the left.  The value under a NULL is that row's.
 *
 * Determinism: the same inputs give the same bytes on every run and every context.  No atomic feeds a result byte (the one
 * atomic is the integer count of tuples of the boundary flags, whose result does not depend on the order of arrival).
 *
 * Limits and errors (*out = NULL): QE_ERR_INVALID_ARG for a null pointer, op outside 0..2, all other than 0 or 1, different
 * column counts, a column whose types differ, zero columns, a STRING column without a dictionary; QE_ERR_UNSUPPORTED for more
 * than 8 columns in a form that sorts (the sort has 8 keys), more than 16 columns in UNION ALL (the limit of
 * qe_result_concat), left rows + right rows >= 2^32 - 1; QE_ERR_HIP on a planning-only context; QE_ERR_OOM when scratch or
 * output does not fit.
 *
 * Zero rows on one side or on both is an ordinary input; the output then may have zero rows and carries the full schema.
 *
 * Lifetime and reuse: the output owns its buffers and shares the dictionaries; both inputs may be freed once the call returns.
 * The output is an ordinary result: qe_result_order_by_keys, qe_batch_from_result, qe_result_to_host, qe_result_concat,
 * qe_gather, the join, the window and another set operation all take it.
 *
 * How: the two sides are concatenated with the placement code of qe_result_concat (right STRING codes through the translation
 * table); one stable sort over every column; the boundary flags of the window operator mark the tuple starts; a bitmap of the
 * sorted positions that hold a left row and its word ranks give cL and cR of every tuple in two lookups, and one pass over the
 * sorted positions, with fixed work per row, writes the keep bitmap; its set positions go through the sort's row ids into the
 * row gather every operator uses.  UNION with all == 0 keeps exactly the tuple starts. */
enum { QE_SET_UNION = 0, QE_SET_INTERSECT = 1, QE_SET_EXCEPT = 2 };
int32_t qe_result_set_op(qe_ctx *ctx, const qe_result *left, const qe_result *right,
                         int32_t op, int32_t all, qe_result **out);
/* what the last qe_result_set_op of this context did: out[0] left rows, out[1] right rows, out[2] distinct tuples of
 * the two sides together found by the sort (0 for UNION ALL: no sort), out[3] STRING columns whose right-side codes were translated
 * into a merged dictionary */
int32_t qe_ctx_last_set_stats(const qe_ctx *ctx, int64_t out[4]);

/* ---- ASOF join of two results -----------------------------------------------------------------------------------
 * For every left row the ONE right row of the same by tuple whose `on` value is nearest at or before it (QE_ASOF_BACKWARD) or
 * at or after it (QE_ASOF_FORWARD): for every trade the last quote of its symbol, for every event the next calibration reading
 * of its sensor.  The hash join (qe_join_build / qe_join_probe) matches on equality only, a window cannot look into another
 * result and the set operations need one schema on both sides.  The reference has no join at all (Query.g4 reads one table).
 *
 * Keys: 0 <= nby <= 7 (the by columns and the `on` column are the sort's 8 keys).  By column i of the left pairs with by
 * column i of the right; the two have the same type, any of the five.  Two by tuples are equal as hash-join keys are
 * (Double.equals: every NaN is one value, -0.0 is not 0.0; STRING compares by string, the sides may carry different
 * dictionaries), and a NULL in any by column, on either side, matches nothing.  nby == 0: the whole input is one partition.
 *
 * The `on` column is DOUBLE, INT64 or INT32, the same type on both sides, and is compared in its own type under the comparator
 * of qe_result_order_by_keys: Double.compareTo for DOUBLE (-0.0 < 0.0, NaN greatest, all NaNs equal), integer order for the
 * integer types -- INT64 values beyond 2^53 never go through a double.  A NULL `on` matches nothing, on either side.
 *
 * The match of a left row l.  Candidates are the right rows r with an equal by tuple and a valid `on`.
 *   QE_ASOF_BACKWARD: cmp(on(r), on(l)) <= 0 (< 0 when strict); of those the greatest on(r); of several with that value the one
 *     with the greatest right row index.
 *   QE_ASOF_FORWARD:  cmp(on(r), on(l)) >= 0 (> 0 when strict); of those the smallest on(r); of several with that value the one
 *     with the smallest right row index.
 * A left row matches exactly one right row, or none.
 *
 * Rows and order.  QE_JOIN_LEFT: one output row per left row, in left input order; where there is no match every right column
 * is NULL (validity 0, value zero).  QE_JOIN_INNER: only the matched left rows, in left input order.
 *
 * Columns: the listed left columns, then the listed right columns.  A column may be listed twice and either list may be empty,
 * but there is at least one output column.  A STRING column carries its source's dictionary (merged dictionaries are scratch
 * for the keys only); nullability is the source's, and under QE_JOIN_LEFT every right column is nullable.  `left` and `right`
 * may be the same handle.
 *
 * Determinism: the same inputs give the same bytes on every run and every context.  No atomic feeds a result byte (the one
 * atomic is the integer count of partitions of the boundary flags).
 *
 * Limits and errors (*out = NULL): QE_ERR_INVALID_ARG for a null pointer (left_by / right_by may be null when nby == 0, a column
 * list when its count is 0), nby outside 0..7, direction outside 0..1, strict other than 0 or 1, a join_type other than
 * QE_JOIN_INNER or QE_JOIN_LEFT, a negative column count, no output column -- these are checked before either result is read --
 * a column out of range, paired by columns of different types, an `on` column that is not DOUBLE, INT64 or INT32 or whose type
 * differs between the sides, a STRING by column without a dictionary; QE_ERR_UNSUPPORTED for left rows + right rows > 2^32 - 2;
 * QE_ERR_HIP on a planning-only context; QE_ERR_OOM when scratch or output does not fit.  Zero rows on either side is an
 * ordinary input and returns the full schema.
 *
 * Lifetime and reuse: the output owns its buffers and shares the dictionaries; both inputs may be freed once the call returns.
 * The output is an ordinary result (qe_batch_from_result, qe_result_order_by_keys, ..).
 *
 * How: the nby + 1 key columns of both sides are concatenated into a scratch result (right STRING codes through the set
 * operations' translation table) -- the right rows first for (BACKWARD, not strict) and (FORWARD, strict), the left rows first
 * for the other two, so that the stable sort over (by.., on) lets ties fall the way the match is defined; the boundary flags of
 * the window operator mark the partition starts; one pass marks the sorted positions whose row is valid in every key, and
 * those of them that hold a right row; a second pass, with fixed work per left row, takes the nearest marked right position
 * before (after) its own from the ranks and positions of that bitmap and accepts it when no partition starts in between.  The
 * row gather every operator uses builds the output. */
enum { QE_ASOF_BACKWARD = 0, QE_ASOF_FORWARD = 1 };
int32_t qe_result_asof_join(qe_ctx *ctx, const qe_result *left, const qe_result *right,
                            const int32_t *left_by, const int32_t *right_by, int32_t nby,
                            int32_t left_on, int32_t right_on,
                            int32_t direction, int32_t strict, int32_t join_type,   /* QE_JOIN_INNER or QE_JOIN_LEFT */
                            const int32_t *left_out, int32_t nleft_out,
                            const int32_t *right_out, int32_t nright_out, qe_result **out);
/* what the last qe_result_asof_join of this context did: out[0] left rows, out[1] right rows, out[2] left rows that found a
 * match, out[3] by partitions the sort found over both sides together (NULL counts as a key value there; 0 when there are no
 * rows at all) */
int32_t qe_ctx_last_asof_stats(const qe_ctx *ctx, int64_t out[4]);

/* ---- range join of two results ----------------------------------------------------------------------------------
 * For every left row ALL right rows of the same by tuple whose `on` value lies in the left row's interval [lo, hi]: all quotes
 * in the five seconds before a trade, all events inside a session, all readings inside a calibration window, a value put into
 * its bin.  The hash join (qe_join_build / qe_join_probe) matches on equality only and walks the matches of one probe row with
 * one lane; the ASOF join returns at most one right row per left row.  The reference has no join at all (Query.g4 reads one
 * table).
 *
 * Keys: 0 <= nby <= 7 (the by columns and one value column are the sort's 8 keys).  By column i of the left pairs with by
 * column i of the right; the two have the same type, any of the five.  Two by tuples are equal as hash-join keys are
 * (Double.equals: every NaN is one value, -0.0 is not 0.0; STRING compares by string, the sides may carry different
 * dictionaries), and a NULL in any by column, on either side, matches nothing.  nby == 0: the whole input is one partition.
 *
 * Interval: left_lo and left_hi (columns of the left) and right_on (a column of the right) are DOUBLE, INT64 or INT32, all three
 * of one type, and are compared in that type under the comparator of qe_result_order_by_keys: Double.compareTo for DOUBLE
 * (-0.0 < 0.0, NaN greatest, all NaNs equal), integer order for the integer types -- INT64 values beyond 2^53 never go through a
 * double.  Right row r matches left row l when the by tuples are equal, cmp(on(r), lo(l)) >= 0 (> 0 when lo_strict) and
 * cmp(on(r), hi(l)) <= 0 (< 0 when hi_strict).  A NULL lo, hi or on matches nothing; an empty interval (lo above hi, or lo
 * equal to hi with a strict end) matches nothing.  left_lo == left_hi (the same column) is allowed: with no strict end it is
 * equality on the value.  The library does no arithmetic on the bounds: a caller derives them with a projection such as t - 5,
 * t + 5 through qe_filter_project and passes the result in.
 *
 * Join types (the values of the hash join's enum).  QE_JOIN_INNER: one row per (left row, matching right row).  QE_JOIN_LEFT:
 * the same, and one row in its place for every left row without a match, every right column of it NULL (validity 0, value
 * zero).  QE_JOIN_SEMI: every left row with at least one match, once.  QE_JOIN_ANTI: every left row without one (a NULL key
 * counts as no match).  SEMI and ANTI take no right columns (nright_out == 0).  QE_JOIN_RIGHT: a HEAD, exactly the rows of
 * QE_JOIN_INNER in their order, then a TAIL: every right row that no left row of this call matched, once, in ascending right
 * row index, every left column of it NULL (validity 0, value zero); a right row with a NULL by column or a NULL on matches
 * nothing and is always in the tail.  QE_JOIN_FULL: the same with the rows of QE_JOIN_LEFT as the head.  Without left rows the
 * tail is the whole right side; without right rows RIGHT is empty and FULL is LEFT.  The values 4 to 7 are unassigned.
 *
 * Order: left rows come out in input order; inside one left row the matches ascend by on(r) under the comparator, ties in
 * ascending right row index.  So with left_lo == left_hi, no strict end, nby == 0 and a key without NULLs the pairs and their
 * order are exactly those of qe_join_probe with the left as probe side.
 *
 * Columns: the listed left columns, then the listed right columns.  A column may be listed twice and either list may be empty,
 * but there is at least one output column.  A STRING column carries its source's dictionary (merged dictionaries are scratch
 * for the keys only); nullability is the source's, and under QE_JOIN_LEFT every right column is nullable, under QE_JOIN_RIGHT
 * every left column, under QE_JOIN_FULL every column.  `left` and `right` may be the same handle.
 *
 * Determinism: the same inputs give the same bytes on every run and every context.  The atomics are an integer max for the
 * stats and, under RIGHT / FULL, integer adds (how many intervals cover a position of the list of right rows) and integer ORs
 * (the marks of the matched right rows), whose final values do not depend on arrival order; no atomic decides a position in
 * the output.
 *
 * Sizes: counts and offsets of the output are 64-bit throughout; the output's size is read back once, as in the hash join,
 * together with the stats and the length of the tail.
 *
 * Limits and errors (*out = NULL): QE_ERR_INVALID_ARG for a null pointer (left_by / right_by may be null when nby == 0, a column
 * list when its count is 0), nby outside 0..7, a strict flag other than 0 or 1, a join_type outside the six, a negative column
 * count, no output column, right columns with SEMI or ANTI -- these are checked before either result is read -- a column out of
 * range, paired by columns of different types, a value column that is not DOUBLE, INT64 or INT32, value columns whose types
 * differ among the three, a STRING by column without a dictionary; QE_ERR_UNSUPPORTED for left rows + right rows > 2^32 - 2;
 * QE_ERR_HIP on a planning-only context; QE_ERR_OOM when scratch or output does not fit.  Zero rows on either side is an
 * ordinary input and returns the full schema.
 *
 * Lifetime and reuse: the output owns its buffers and shares the dictionaries; both inputs may be freed once the call returns.
 * The output is an ordinary result (qe_batch_from_result, qe_result_order_by_keys, another range join, ..).
 *
 * How: two stable sorts over the concatenated key columns of both sides (right STRING codes through the set operations'
 * translation table), one with lo and one with hi as the left rows' value next to the right rows' on; the order of the
 * concatenation lets ties fall the way the two ends are defined.  In each sort a left row reads off its ORDINAL, the number of
 * right rows with a whole key before it.  Those right rows stand in the same order in both sorts, so the two ordinals index one
 * list and the matches of a left row are the entries between them.  A 64-bit scan of the per-row counts gives every left row
 * its first output row, and a load-balanced expansion -- a workgroup per tile of consecutive OUTPUT rows, a search per output
 * row, no lane walking one left row's matches -- writes the row pairs for the row gather every operator uses.  RIGHT / FULL: the
 * matched right rows are the union of those index intervals; +1 / -1 at their ends in a difference array, one more scan and a
 * marking pass give the bitmap of the matched right rows, and its complement, compacted, is the tail. */
int32_t qe_result_range_join(qe_ctx *ctx, const qe_result *left, const qe_result *right,
                             const int32_t *left_by, const int32_t *right_by, int32_t nby,
                             int32_t left_lo, int32_t left_hi, int32_t right_on,
                             int32_t lo_strict, int32_t hi_strict, int32_t join_type,   /* QE_JOIN_INNER / LEFT / SEMI / ANTI / RIGHT / FULL */
                             const int32_t *left_out, int32_t nleft_out,
                             const int32_t *right_out, int32_t nright_out, qe_result **out);
/* what the last qe_result_range_join of this context did: out[0] left rows, out[1] right rows, out[2] output rows, out[3] the
 * most matches any one left row has */
int32_t qe_ctx_last_range_stats(const qe_ctx *ctx, int64_t out[4]);

/* zero-copy: a batch whose columns ARE the result's (not owned; the result must outlive the batch).  Same columns, same
 * validity (NULL where the result has none), same dictionaries, nrows = the result's count (zero rows: a zero-row batch).
 * The batch goes into qe_filter_project / qe_filter_aggregate / qe_filter_groupby like any other: that is how a join is
 * followed by a GROUP BY, a filter (HAVING) or a projection without leaving HBM.  qe_batch_free frees only the handle.  A
 * qe_result_free that comes while such a batch is alive does not pull the buffers from under it: they are released when
 * the result's last batch is freed (the result handle itself must not be used after qe_result_free all the same). */
int32_t qe_batch_from_result(qe_ctx *ctx, const qe_result *result, qe_batch **out);

/* ---- the exchange step of a row-range sharded scan -------------------------------------------------------
 * One process (one qe_ctx) per GPU; rank r scans rows [r*N/P, (r+1)*N/P) with NO communication.  Only a plan whose root
 * materialises its result on one rank (evaluator/Planner.kt:30-63: ONE Operator yields the whole result; Main.kt:18
 * `physicalPlan.map { it }`) exchanges data.  RCCL directly: ncclAllGather of the per-rank result headers, then one
 * ncclGroupStart/End of ncclRecv (root, at the final offsets) / ncclSend (peers), every peer on its own xGMI link;
 * rank order = the reference's row order (operator/FilterOperator.kt:17-22 is order preserving).
 * Bootstrap: rank 0 calls qe_comm_unique_id and hands the 128 bytes to the other ranks through whatever channel the
 * host has (the JVM host: its own RPC; tests / bench.py: torch.distributed broadcast); then every rank calls
 * qe_comm_init.  Failures return QE_ERR_COMM. */
typedef struct { char internal[128]; } qe_comm_id;     /* = ncclUniqueId */
int32_t qe_comm_unique_id(qe_ctx *ctx, qe_comm_id *out);
int32_t qe_comm_init(qe_ctx *ctx, int32_t nranks, int32_t rank, const qe_comm_id *id);
int32_t qe_comm_rank(const qe_ctx *ctx);       /* -1 without a communicator */
int32_t qe_comm_nranks(const qe_ctx *ctx);     /* 0 without a communicator */
void qe_comm_destroy(qe_ctx *ctx);             /* also done by qe_ctx_destroy */
/* Collective.  On `root`, *out = the concatenation of every rank's result in rank order (free with qe_result_free);
 * on the other ranks *out = NULL.  `local` stays owned by the caller.
 * Every rank must hold a result of the same shape (same plan): column count and types are compared on every rank, and a
 * STRING column must carry THE SAME DICTIONARY (same entries, same order) on every rank -- codes travel, not strings, and
 * the root labels them with its own dictionary.  A host that parses each shard's text separately (qe_csv_parse_file per
 * rank) gets a first-appearance dictionary per shard and must pin ONE shared dictionary instead.  A mismatch is
 * QE_ERR_INVALID_ARG on EVERY rank (the fingerprints travel in the header all-gather), as is a schema mismatch; a rank that
 * cannot allocate its buffers makes the call fail on every rank before any transfer starts (QE_ERR_OOM). */
int32_t qe_gather(qe_ctx *ctx, const qe_result *local, int32_t root, qe_result **out);
/* Collective: Projection(Filter(Scan)) over this rank's shard AND the materialising exchange in one call, OVERLAPPED -- the
 * shard is scanned in `nslices` slices (<= 16; 0 = 8) and a slice's rows travel to the root (copy stream) while the next slice
 * is scanned (compute stream).  The root can only place rows at their final offset if every count is known in advance: the
 * call starts with a count pre-pass (the filter's columns only) and ONE all-gather of every rank's per-slice counts.  Same
 * result, order and checks as qe_filter_project + qe_gather.  On `root` *out = the whole result, elsewhere NULL. */
int32_t qe_filter_project_gather(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter, const qe_expr *const *projections,
                                 int32_t nproj, int32_t root, int32_t nslices, qe_result **out);
/* Collective, small control data (aggregate partials, counts): recv gets nranks * nbytes host bytes in rank order.
 * Aggregations over a sharded table fold the per-GPU partials in rank order on the host. */
int32_t qe_comm_allgather_host(qe_ctx *ctx, const void *send, size_t nbytes, void *recv);

/* ---- introspection ------------------------------------------------------------------------ */
/* HIP source the JIT would compile for this plan (NUL terminated, owned by ctx, valid until next call) */
int32_t qe_filter_project_source(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                 const qe_expr *const *projections, int32_t nproj, const char **out);
/* Which of the fused kernel's three geometries this plan runs with on large batches: -1 not decided yet (the first
 * executions on a batch of >= 32 Mi rows time all three, best of 3 each), 0 default, 1 wide (16 load groups per sub-tile,
 * 512-entry LDS rings, 2 waves per SIMD), 2 mid (the default sub-tile, 8 Ki-row chunks, 512-entry rings, 2 waves per
 * workgroup).  The decision is persisted next to the plan's code object in the JIT cache, so a later context / process runs the
 * same geometry without exploring (*out_from_cache = 1 when it came from there) -- unless the winner was less than 7 % ahead
 * (the spread of one binary over the boxes of a pool): such a decision is measured again once per context. */
int32_t qe_filter_project_geometry(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                   const qe_expr *const *projections, int32_t nproj, int32_t *out_chosen,
                                   int32_t *out_from_cache);
/* The order in which this plan evaluates the conjuncts of its filter's top-level AND chain (and so loads their columns):
 * out_order[k] = index, in WRITTEN order, of the conjunct evaluated k-th.  *out_nconj = number of conjuncts, or -1 while
 * the plan has not measured yet (its first execution on a batch of >= 8 Mi rows measures every conjunct's pass rate and
 * keeps the order that fetches the fewest lines; smaller batches run as written).  The reference's AND is lazy left to
 * right (evaluator/Interpreter.kt:54-72) -- with typed plans and no side effects any order keeps the same rows. */
int32_t qe_filter_project_conjunct_order(qe_ctx *ctx, const qe_batch *batch, const qe_expr *filter,
                                         const qe_expr *const *projections, int32_t nproj, int32_t *out_order, int32_t capacity,
                                         int32_t *out_nconj);
/* Which form the last qe_filter_project / qe_filter_groupby on this context ran in (-1: none yet).  The fused executor picks the form from the
 * share of rows the plan kept last time: the local form up to 3 % (large batches), the LDS-ring single pass below 12 %, the
 * dense single pass from there on. */
enum { QE_FORM_RING = 0, QE_FORM_TWO_PASS = 1, QE_FORM_DENSE = 2, QE_FORM_PER_NODE = 3, QE_FORM_NO_FILTER = 4,
       QE_FORM_LOCAL = 5 /* dependency-free scan into per-chunk slots + one move: plans that kept <= 3 % of their rows */,
       /* qe_filter_groupby: */ QE_FORM_GROUPBY_DENSE = 8, QE_FORM_GROUPBY_HASHED = 9,
       QE_FORM_GROUPBY_HASH_PARTITIONED = 10 /* many distinct numeric keys: rows scattered by key hash, an LDS hash table per partition */ };
int32_t qe_ctx_last_form(const qe_ctx *ctx);
/* measured device read bandwidth of a plain streaming kernel over nbytes (GB/s): roofline calibration */
int32_t qe_stream_read_bandwidth(qe_ctx *ctx, int64_t nbytes, int32_t reps, double *out_gbps);

/* calibration: time (ms) of streaming nbytes with one 512-byte block WRITTEN per wave every `write_every`
 * 8-KiB read iterations (0 = read only); what a trickle of writes costs a read stream on this device */
int32_t qe_stream_read_write_time(qe_ctx *ctx, int64_t nbytes, int32_t write_every, int32_t reps, double *out_ms,
                                  double *out_written_bytes);

#ifdef __cplusplus
}
#endif
#endif
