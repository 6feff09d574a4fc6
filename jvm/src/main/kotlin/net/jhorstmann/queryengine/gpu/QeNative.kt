// Reference-side binding of libqe_hip.so (include/qe_hip.h) through the Java Foreign Function &
// Memory API (JDK >= 22).  NOT compiled in this repository: the build image has no JDK/kotlinc
// (SURVEY.md 8c).  It shows exactly which symbols the Kotlin side binds and how; a JNI shim with
// the same calls is the alternative for the reference's Java 11 target (pom.xml:13-15).
package net.jhorstmann.queryengine.gpu

import java.lang.foreign.*
import java.lang.foreign.ValueLayout.*
import java.lang.invoke.MethodHandle

internal object QeNative {
    private val linker = Linker.nativeLinker()
    private val lib = SymbolLookup.libraryLookup(System.getProperty("qe.hip.library", "libqe_hip.so"), Arena.global())

    private fun handle(name: String, res: MemoryLayout?, vararg args: MemoryLayout): MethodHandle {
        val fd = if (res == null) FunctionDescriptor.ofVoid(*args) else FunctionDescriptor.of(res, *args)
        return linker.downcallHandle(lib.find(name).orElseThrow { UnsatisfiedLinkError(name) }, fd)
    }

    val qe_last_error = handle("qe_last_error", ADDRESS, ADDRESS)
    val qe_ctx_create = handle("qe_ctx_create", JAVA_INT, JAVA_INT, ADDRESS, ADDRESS)
    val qe_ctx_destroy = handle("qe_ctx_destroy", null, ADDRESS)
    val qe_dict_create = handle("qe_dict_create", JAVA_INT, ADDRESS, JAVA_INT, ADDRESS, ADDRESS)
    val qe_dict_size = handle("qe_dict_size", JAVA_INT, ADDRESS)
    val qe_dict_entry = handle("qe_dict_entry", ADDRESS, ADDRESS, JAVA_INT)
    val qe_batch_create = handle("qe_batch_create", JAVA_INT, ADDRESS, JAVA_LONG, JAVA_INT, ADDRESS, ADDRESS)
    val qe_batch_free = handle("qe_batch_free", null, ADDRESS, ADDRESS)
    val qe_expr_compile = handle("qe_expr_compile", JAVA_INT, ADDRESS, ADDRESS, JAVA_LONG, ADDRESS)
    val qe_expr_free = handle("qe_expr_free", null, ADDRESS, ADDRESS)
    val qe_filter_project = handle("qe_filter_project", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, ADDRESS)
    val qe_filter_project_prepare = handle("qe_filter_project_prepare", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT)
    val qe_filter_aggregate = handle("qe_filter_aggregate", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT,
            ADDRESS, ADDRESS, ADDRESS)
    // ctx, batch, filter|NULL, qe_expr*[nkeys], nkeys, qe_expr*[nagg], int32 fns[nagg], nagg, qe_result** -> status
    val qe_filter_groupby = handle("qe_filter_groupby", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS,
            JAVA_INT, ADDRESS)
    val qe_ctx_last_groupby_stats = handle("qe_ctx_last_groupby_stats", JAVA_INT, ADDRESS, ADDRESS)   // ctx, long[4]: route, abandoned launches, capacity, partitions
    val qe_result_count = handle("qe_result_count", JAVA_LONG, ADDRESS)
    val qe_result_ncols = handle("qe_result_ncols", JAVA_INT, ADDRESS)
    val qe_result_column = handle("qe_result_column", JAVA_INT, ADDRESS, JAVA_INT, ADDRESS)
    val qe_result_column_to_host = handle("qe_result_column_to_host", JAVA_INT, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS)
    val qe_result_free = handle("qe_result_free", null, ADDRESS, ADDRESS)
    // result -> PINNED host memory owned by the library (pooled per context), on the context's copy stream:
    // qe_result_to_host STARTS the copies and returns; wait blocks; column gives HOST pointers in a qe_col_view
    val qe_result_to_host = handle("qe_result_to_host", JAVA_INT, ADDRESS, ADDRESS, ADDRESS)          // ctx, result, qe_host_result**
    val qe_host_result_wait = handle("qe_host_result_wait", JAVA_INT, ADDRESS, ADDRESS)
    val qe_host_result_count = handle("qe_host_result_count", JAVA_LONG, ADDRESS)
    val qe_host_result_ncols = handle("qe_host_result_ncols", JAVA_INT, ADDRESS)
    val qe_host_result_column = handle("qe_host_result_column", JAVA_INT, ADDRESS, JAVA_INT, ADDRESS) // host, col, qe_col_view*
    val qe_host_result_free = handle("qe_host_result_free", null, ADDRESS, ADDRESS)
    // ctx, qe_result*[nparts], nparts, qe_result** -> status: results of consecutive batches as ONE result (input order)
    val qe_result_concat = handle("qe_result_concat", JAVA_INT, ADDRESS, ADDRESS, JAVA_INT, ADDRESS)
    // ctx, result, column (0-based), qe_result** -> status: OrderByOperator.kt:9-15 on the device
    val qe_result_order_by = handle("qe_result_order_by", JAVA_INT, ADDRESS, ADDRESS, JAVA_INT, ADDRESS)
    // ctx, result, qe_sort_key[nkeys] {int column, int descending}, nkeys, limit (< 0: none), qe_result** -> status:
    // compareBy().thenByDescending() on a stable sort, LIMIT as a top-k selection on the device
    val qe_result_order_by_keys = handle("qe_result_order_by_keys", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, JAVA_LONG, ADDRESS)

    // ---- hash equi-join of two device-resident sides; a side is a qe_join_input {qe_result*, qe_batch*}, exactly one set ----
    // ctx, build side, int key_cols[nkeys], nkeys (1..4), qe_join_table** -> status; the build side must outlive the table
    val qe_join_build = handle("qe_join_build", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, ADDRESS)
    val qe_join_table_rows = handle("qe_join_table_rows", JAVA_LONG, ADDRESS)                         // build rows with a key
    val qe_join_table_free = handle("qe_join_table_free", null, ADDRESS, ADDRESS)
    // ctx, table, probe side, int key_cols[nkeys], nkeys, join type (0 INNER, 1 LEFT, 2 SEMI, 3 ANTI, 8 RIGHT, 9 FULL), int probe_out[n], n,
    // int build_out[m], m (0 for SEMI / ANTI), qe_result** -> status: rows in nested-loop order, probe side outside
    val qe_join_probe = handle("qe_join_probe", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS)
    val qe_ctx_last_join_stats = handle("qe_ctx_last_join_stats", JAVA_INT, ADDRESS, ADDRESS)         // ctx, long[4]
    val qe_ctx_last_outer_stats = handle("qe_ctx_last_outer_stats", JAVA_INT, ADDRESS, ADDRESS)       // ctx, long[4]: 1 hash / 2 range, head rows, tail rows, matched build / right rows
    // ---- window functions over a result (ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW inside the partition) ----
    // ctx, result, int partition_cols[npart], npart, qe_sort_key order[norder], norder, qe_window_fn fns[nfn] {int fn, int column,
    // long offset}, nfn (1..16), qe_result** -> status: every input column sorted by (partition, order), then one column per function
    // (fn: 0 ROW_NUMBER, 1 RANK, 2 DENSE_RANK, 3 SUM, 4 COUNT, 5 MIN, 6 MAX, 7 AVG, 8 LAG, 9 LEAD)
    val qe_result_window = handle("qe_result_window", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS)
    // the same with a frame per function: qe_window_frame_fn fns[nfn] {int fn, int column, long offset, long preceding, long following}
    // (ROWS BETWEEN preceding PRECEDING AND following FOLLOWING, -1 = UNBOUNDED; fn 10 / 11 = FIRST_VALUE / LAST_VALUE), qe_result **out
    val qe_result_window_frames = handle("qe_result_window_frames", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS)
    val qe_ctx_last_window_stats = handle("qe_ctx_last_window_stats", JAVA_INT, ADDRESS, ADDRESS)     // ctx, long[4]
    // ---- set operations over two results of one schema: op 0 UNION, 1 INTERSECT, 2 EXCEPT; all 0 / 1 (the multiset form) ----
    // ctx, left, right, op, all, qe_result** -> status: NULL equals NULL, strings compare by string (the sides may carry different
    // dictionaries); UNION ALL is left's rows then right's, every other form ascending by all columns
    val qe_result_set_op = handle("qe_result_set_op", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, JAVA_INT, ADDRESS)
    val qe_ctx_last_set_stats = handle("qe_ctx_last_set_stats", JAVA_INT, ADDRESS, ADDRESS)           // ctx, long[4]
    // ---- ASOF join of two results: direction 0 BACKWARD (nearest at or before), 1 FORWARD (at or after); strict 0 / 1; join_type 0 INNER, 1 LEFT ----
    // ctx, left, right, int[] left_by, int[] right_by, nby (0..7), left_on, right_on, direction, strict, join_type, int[] left_out, nleft_out,
    // int[] right_out, nright_out, qe_result** -> status: per left row the one right row of its by tuple with the nearest `on`, in left row order
    val qe_result_asof_join = handle("qe_result_asof_join", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, JAVA_INT, JAVA_INT,
        JAVA_INT, JAVA_INT, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS)
    val qe_ctx_last_asof_stats = handle("qe_ctx_last_asof_stats", JAVA_INT, ADDRESS, ADDRESS)         // ctx, long[4]
    // ---- range join of two results: lo_strict / hi_strict 0 / 1 exclude that end; join_type 0 INNER, 1 LEFT, 2 SEMI, 3 ANTI ----
    // ctx, left, right, int[] left_by, int[] right_by, nby (0..7), left_lo, left_hi, right_on, lo_strict, hi_strict, join_type, int[] left_out,
    // nleft_out, int[] right_out, nright_out (0 for SEMI / ANTI), qe_result** -> status: per left row all right rows of its by tuple with on in
    // [lo, hi], in left row order, the matches of one left row ascending by on
    val qe_result_range_join = handle("qe_result_range_join", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, JAVA_INT, JAVA_INT,
        JAVA_INT, JAVA_INT, JAVA_INT, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS, JAVA_INT, ADDRESS)
    val qe_ctx_last_range_stats = handle("qe_ctx_last_range_stats", JAVA_INT, ADDRESS, ADDRESS)       // ctx, long[4]: left rows, right rows, output rows, longest
    // ctx, result, qe_batch** -> status: a batch whose columns ARE the result's (zero copy): the input of the next plan
    val qe_batch_from_result = handle("qe_batch_from_result", JAVA_INT, ADDRESS, ADDRESS, ADDRESS)

    // ---- the exchange step of a row-range sharded scan: one JVM process (one qe_ctx) per GPU ----
    // rank 0: qe_comm_unique_id(ctx, id128) -> the 128 bytes travel to the other ranks over the host's own channel
    val qe_comm_unique_id = handle("qe_comm_unique_id", JAVA_INT, ADDRESS, ADDRESS)
    val qe_comm_init = handle("qe_comm_init", JAVA_INT, ADDRESS, JAVA_INT, JAVA_INT, ADDRESS)       // ctx, nranks, rank, id128
    val qe_comm_rank = handle("qe_comm_rank", JAVA_INT, ADDRESS)
    val qe_comm_nranks = handle("qe_comm_nranks", JAVA_INT, ADDRESS)
    val qe_comm_destroy = handle("qe_comm_destroy", null, ADDRESS)
    // collective: ctx, local result, root, qe_result** (non-NULL on root only) -> status (QE_ERR_COMM = 7 on an RCCL failure)
    val qe_gather = handle("qe_gather", JAVA_INT, ADDRESS, ADDRESS, JAVA_INT, ADDRESS)
    // collective: ctx, batch, filter|NULL, qe_expr*[nproj], nproj, root, nslices (0 = 8), qe_result** -> scan + exchange overlapped
    val qe_filter_project_gather = handle("qe_filter_project_gather", JAVA_INT, ADDRESS, ADDRESS, ADDRESS, ADDRESS, JAVA_INT, JAVA_INT, JAVA_INT, ADDRESS)
    // collective: ctx, send, nbytes, recv[nranks * nbytes] (host buffers): aggregate partials, counts
    val qe_comm_allgather_host = handle("qe_comm_allgather_host", JAVA_INT, ADDRESS, ADDRESS, JAVA_LONG, ADDRESS)

    // ---- CSV text -> columns (replaces CsvTable / UnivocityCsvTable scan leaves) ----
    // ctx, path, nfields, char*[names], int32[types], qe_csv_table** -> status
    val qe_csv_parse_file = handle("qe_csv_parse_file", JAVA_INT, ADDRESS, ADDRESS, JAVA_INT, ADDRESS, ADDRESS, ADDRESS)
    val qe_csv_nrows = handle("qe_csv_nrows", JAVA_LONG, ADDRESS)
    val qe_csv_column = handle("qe_csv_column", JAVA_INT, ADDRESS, JAVA_INT, ADDRESS)                  // -> qe_col_desc (host pointers)
    val qe_csv_pin = handle("qe_csv_pin", JAVA_INT, ADDRESS, ADDRESS, ADDRESS)                          // -> qe_batch (HBM)
    val qe_csv_free = handle("qe_csv_free", null, ADDRESS, ADDRESS)

    /** struct qe_col_desc { int32 type; int32 reserved; const void* data; const uint64* validity; const qe_dict* dict; } */
    val COL_DESC: StructLayout = MemoryLayout.structLayout(
            JAVA_INT.withName("type"), JAVA_INT.withName("reserved"),
            ADDRESS.withName("data"), ADDRESS.withName("validity"), ADDRESS.withName("dict"))

    /** struct qe_col_view { int32 type; int32 nullable; const void* data; const uint64* validity; int64 count; const qe_dict* dict; } */
    val COL_VIEW: StructLayout = MemoryLayout.structLayout(
            JAVA_INT.withName("type"), JAVA_INT.withName("nullable"),
            ADDRESS.withName("data"), ADDRESS.withName("validity"), JAVA_LONG.withName("count"), ADDRESS.withName("dict"))

    fun check(ctx: MemorySegment, status: Int) {
        if (status != 0) {
            val msg = (qe_last_error.invokeExact(ctx) as MemorySegment).reinterpret(4096).getString(0)
            throw when (status) {
                1 -> IllegalArgumentException(msg)
                2 -> net.jhorstmann.queryengine.evaluator.TypeCheckException(msg)
                else -> IllegalStateException("libqe_hip status $status: $msg")
            }
        }
    }
}
