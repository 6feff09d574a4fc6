"""qe_result_group_ordered on the device: COUNT_DISTINCT, PERCENTILE_CONT / DISC and MODE per group, and SELECT DISTINCT.

The expectation is tests/ordered_reference.py (numpy; proved equal to the host branch of ``OrderedAggregateOperator`` in
tests/test_ordered_cpu.py).  Every output column is compared in full -- type, nullability, dictionary, validity, values by
bits, PERCENTILE_CONT included (the comparison takes any NaN for any NaN: the header leaves a NaN's payload to the formula) --
and the value under every NULL must be zero.  There is no tolerance anywhere.  Sizes are those where the kernels change
behaviour: word (64) and tile (2048) edges of the bitmaps, more than one 1024-word block of the word-rank scan (the shared
scan's own trips and sweeps are tested at their seams in tests/scan), and the grid cap native.OSA_BLOCKS (a lane per group or run).

One error of the contract has no test: a STRING column without a dictionary cannot be built through the ABI."""
import ctypes as C

import numpy as np
import pytest

from queryengine_amd import AggregationFunction as AF
from queryengine_amd import Column, ColumnExpression, DataType, Function, FunctionExpression, NumericLiteralExpression
from queryengine_amd import engine as E
from queryengine_amd import native as N

from ordered_reference import ordered_reference
from window_reference import T, TRIP, assert_window_output, window_reference

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
CD, CONT, DISC, MODE = N.OSA_COUNT_DISTINCT, N.OSA_PERCENTILE_CONT, N.OSA_PERCENTILE_DISC, N.OSA_MODE
INVALID_ARG, HIP = 1, 3
NAN, INF = float("nan"), float("inf")
FRACTIONS = [0.0, 0.25, 1 / 3, 0.5, 2 / 3, 0.999, 1.0]
STRINGS = ["b", "a", "", "B", "～", "\U0001F600", "aa", "Zü", "zz", "a "]     # not in sorted order
SEAM_N = 3 * T + 37
SEAM_LENGTHS = [1, 2, 63, 64, 65, 512, 513, 2048, 2049]
BIG = TRIP * T + 321            # 32 blocks of the word-rank scan and a ragged tail; also past OSA_WORD_BLOCKS * 256 words
GROUP_CAP = N.OSA_BLOCKS * 256  # lanes of one sweep of the per-group and per-run kernels
assert BIG > N.OSA_WORD_BLOCKS * 256 * 64 and BIG // 64 > 1024


def build(ctx, cols):
    """filter_project over an identity projection: a result that holds exactly `cols`."""
    batch = E.DeviceBatch.from_columns(ctx, cols)
    projs = [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)]
    return batch, E.filter_project(ctx, batch, None, projs)


def run_case(ctx, cols, group_by, fns, what, res=None, sorts=None):
    """One qe_result_group_ordered against the reference; returns (expected columns, groups)."""
    batch = None
    if res is None:
        batch, res = build(ctx, cols)
    try:
        nullable = [bool(res.view(c).nullable) for c in range(res.ncols)]
        want, groups = ordered_reference(cols, nullable, group_by, fns)
        out = ctx.group_ordered(res, group_by, fns)
        try:
            stats = ctx.last_ordered_stats()
            assert out.count == groups, (what, out.count, groups)
            assert_window_output(out, want, what)
            distinct_args = len({f[1] for f in fns}) or 1
            assert stats["rows"] == len(cols[0]) and stats["groups"] == groups, (what, stats, groups)
            assert stats["sorts"] == (0 if len(cols[0]) == 0 else distinct_args if sorts is None else sorts), (what, stats)
        finally:
            out.free()
    finally:
        if batch is not None:
            res.free(); batch.free()
    return want, groups


def all_four(column, q=0.5, cont=True):
    return [(CD, column), (DISC, column, q), (MODE, column)] + ([(CONT, column, q)] if cont else [])


def column_bytes(result):
    return [(c.data.tobytes(), None if c.valid is None else c.valid.tobytes()) for c in result.to_columns()]


# ---- seams -------------------------------------------------------------------------------------------------------------------------
def seam_columns(rng):
    """(group id, DOUBLE, INT64, INT32, STRING, BOOLEAN): groups of the seam lengths, each with no, some or only NULLs in every
    argument column; the first group is 128 rows of which exactly 64 are NULL, so its first valid row stands on a word edge."""
    lengths = [128]
    while sum(lengths) < SEAM_N:
        lengths.append(SEAM_LENGTHS[rng.integers(0, len(SEAM_LENGTHS))])
    n = SEAM_N
    gid = np.repeat(np.arange(len(lengths)), lengths)[:n].astype(np.int64)
    share = np.array([0.0, 0.3, 1.0])[rng.integers(0, 3, len(lengths))][gid]

    def valid():
        v = rng.random(n) >= share
        v[:128] = np.arange(128) >= 64
        return v
    shuffle = rng.permutation(n)
    cols = [Column(I64, gid),
            Column(D, np.where(rng.random(n) < 0.1, np.array([NAN, INF, -INF, -0.0, 0.0])[rng.integers(0, 5, n)], rng.integers(-20, 20, n) / 4.0), valid()),
            Column(I64, np.where(rng.random(n) < 0.3, 2 ** 53 + rng.integers(-2, 3, n), rng.integers(-9, 9, n)), valid()),
            Column(I32, rng.integers(-6, 6, n).astype(np.int32), valid()),
            Column(S, rng.integers(0, len(STRINGS), n).astype(np.int32), valid(), STRINGS),
            Column(B, rng.random(n) > 0.4, valid())]
    return [Column(c.type, c.data[shuffle], None if c.valid is None else c.valid[shuffle], c.dictionary) for c in cols]


def test_every_function_on_every_type_across_word_and_tile_edges(gpu_ctx):
    rng = np.random.default_rng(61)
    cols = seam_columns(rng)
    assert len(cols[0]) % 64 != 0
    fns = all_four(1, 0.5) + all_four(2, 1 / 3) + all_four(3, 0.999) + all_four(4, 0.25, cont=False) + [(MODE, 5)]
    assert len(fns) == 16
    want, groups = run_case(gpu_ctx, cols, [0], fns, "seams", sorts=5)
    assert (~want[2].valid).any() and groups > 8                                          # groups with c == 0 among them
    run_case(gpu_ctx, cols, [0], all_four(5, 2 / 3, cont=False) + [(DISC, 5, 0.0), (DISC, 5, 1.0)], "seams, BOOLEAN", sorts=1)


# ---- extremes of G ---------------------------------------------------------------------------------------------------------------
def test_every_row_its_own_group(gpu_ctx):
    rng = np.random.default_rng(62)
    n = T + 1
    cols = [Column(I64, rng.permutation(n).astype(np.int64)), Column(D, rng.normal(0, 10, n), rng.random(n) > 0.2)]
    _, groups = run_case(gpu_ctx, cols, [0], all_four(1), "G = n")
    assert groups == n


def test_more_groups_and_runs_than_one_sweep_of_the_per_group_kernels(gpu_ctx):
    """native.OSA_BLOCKS blocks of 256 lanes: with one group (and one run) per row the strided loops take a second trip."""
    rng = np.random.default_rng(63)
    n = GROUP_CAP + 77
    cols = [Column(I32, rng.permutation(n).astype(np.int32)), Column(D, rng.integers(-99, 99, n) / 2.0, rng.random(n) > 0.1)]
    _, groups = run_case(gpu_ctx, cols, [0], all_four(1, 0.25), "G past the cap")
    assert groups == n > N.OSA_BLOCKS * 256


@pytest.mark.parametrize("n", [1, 64, 65, 2 * T + 1])
def test_one_group_without_group_columns(gpu_ctx, n):
    rng = np.random.default_rng(64 + n)
    cols = [Column(D, rng.integers(-30, 30, n) / 8.0, rng.random(n) > 0.3 if n > 1 else None), Column(S, rng.integers(0, len(STRINGS), n).astype(np.int32), None, STRINGS)]
    _, groups = run_case(gpu_ctx, cols, [], all_four(0, 0.5) + all_four(1, 0.999, cont=False) + [(CONT, 0, q) for q in FRACTIONS], f"one group, n {n}")
    assert groups == 1


def test_null_nan_and_signed_zero_group_keys(gpu_ctx):
    rng = np.random.default_rng(65)
    n = 1000
    nan2 = np.frombuffer(np.uint64(0x7ff8000000000123).tobytes(), dtype=np.float64)[0]       # another NaN: the same key
    key = np.array([NAN, nan2, 0.0, -0.0, 1.0, INF])[rng.integers(0, 6, n)]
    cols = [Column(D, key, rng.random(n) > 0.1), Column(I32, rng.integers(0, 9, n).astype(np.int32), rng.random(n) > 0.2)]
    want, groups = run_case(gpu_ctx, cols, [0], all_four(1), "special keys")
    assert groups == 6                                                                       # NULL, -0.0, 0.0, 1.0, inf, NaN
    assert not want[0].valid[0] and np.signbit(want[0].data[1]) and not np.signbit(want[0].data[2]) and np.isnan(want[0].data[5])


# ---- fractions -------------------------------------------------------------------------------------------------------------------
COUNTS = [1, 2, 3, 4, 63, 64, 65]


@pytest.mark.parametrize("kind", ["fractional", "int64-around-2^53", "inf-nan"])
def test_fractions_on_small_and_word_sized_groups(gpu_ctx, kind):
    rng = np.random.default_rng(66)
    gid = np.repeat(np.arange(len(COUNTS) * 3), COUNTS * 3).astype(np.int32)
    n = len(gid)
    if kind == "fractional":
        arg = Column(D, 10.0 ** rng.uniform(-3, 3, n) * rng.choice([-1.0, 1.0], n), rng.random(n) > 0.05)
    elif kind == "int64-around-2^53":                          # as doubles 2^53 and 2^53 + 1 are one value: the sort comes first
        arg = Column(I64, rng.choice([-1, 1], n) * (2 ** 53 + rng.integers(-3, 4, n)), rng.random(n) > 0.05)
    else:
        arg = Column(D, np.array([INF, -INF, NAN, 1.0, 2.5, -0.0])[rng.integers(0, 6, n)])
    shuffle = rng.permutation(n)
    cols = [Column(I32, gid[shuffle]), Column(arg.type, arg.data[shuffle], None if arg.valid is None else arg.valid[shuffle])]
    run_case(gpu_ctx, cols, [0], [(CONT, 1, q) for q in FRACTIONS] + [(DISC, 1, q) for q in FRACTIONS] + [(CD, 1), (MODE, 1)], kind)


def test_the_median_of_two_equal_infinities_is_that_infinity(gpu_ctx):
    cols = [Column(I32, np.array([0, 0, 1, 1, 2, 2, 3], dtype=np.int32)), Column(D, np.array([INF, INF, -INF, -INF, -INF, INF, NAN]))]
    want, _ = run_case(gpu_ctx, cols, [0], [E.MEDIAN(1)], "infinities")
    assert want[1].data[0] == INF and want[1].data[1] == -INF and np.isnan(want[1].data[2]) and np.isnan(want[1].data[3])


# ---- MODE ------------------------------------------------------------------------------------------------------------------------
def test_mode_ties_long_runs_and_many_runs(gpu_ctx):
    rng = np.random.default_rng(67)
    # group 0: runs of equal length, the smallest value wins; group 1: one run of 5000 rows; group 2: a run from row 2040 to
    # row 2060 of the group and a longer one that crosses a tile edge of the whole input
    g0 = np.repeat([7.0, -3.0, 5.0, -0.0, 0.0], 3)
    g1 = np.full(5000, 2.5)
    g2 = np.concatenate([np.arange(2040) * 1.0, np.full(21, 5000.0), np.full(3000, 6000.0), np.arange(100) + 7000.0])
    val = np.concatenate([g0, g1, g2])
    gid = np.concatenate([np.zeros(len(g0)), np.ones(len(g1)), np.full(len(g2), 2)]).astype(np.int32)
    shuffle = rng.permutation(len(val))
    cols = [Column(I32, gid[shuffle]), Column(D, val[shuffle])]
    want, _ = run_case(gpu_ctx, cols, [0], [(MODE, 1), (CD, 1)], "mode")
    assert list(want[1].data) == [-3.0, 2.5, 6000.0] and list(want[2].data) == [5.0, 1.0, 2040 + 102]


def test_mode_of_one_group_with_4096_runs_of_length_one(gpu_ctx):
    """Every run of the input raises the same best[] entry: the same-address path of the integer max."""
    rng = np.random.default_rng(68)
    cols = [Column(I64, rng.permutation(4096).astype(np.int64))]
    want, _ = run_case(gpu_ctx, cols, [], [(MODE, 0), (CD, 0)], "4096 runs")
    assert want[0].data[0] == 0 and want[1].data[0] == 4096.0
    cols = [Column(I32, np.zeros(4096, dtype=np.int32)), Column(I64, np.concatenate([rng.permutation(4094), [77, 77]]).astype(np.int64))]
    want, _ = run_case(gpu_ctx, cols, [0], [(MODE, 1)], "4094 runs of one and one of three")
    assert want[1].data[0] == 77


# ---- the one large case ----------------------------------------------------------------------------------------------------------
def test_one_trip_of_the_tile_scan_and_a_ragged_tail(gpu_ctx):
    """BIG rows in about 100 000 groups, integer-valued DOUBLE data: the reference in full, and two independent cross-checks --
    PERCENTILE_DISC(0) / (1) are MIN / MAX of qe_filter_groupby matched by key, COUNT_DISTINCT is the last DENSE_RANK of
    qe_result_window of every partition."""
    ctx = gpu_ctx
    rng = np.random.default_rng(69)
    n = BIG
    cols = [Column(I64, rng.integers(0, 100_000, n)), Column(D, rng.integers(-40, 40, n).astype(np.float64), rng.random(n) > 0.05)]
    batch, res = build(ctx, cols)
    fns = all_four(1) + [(DISC, 1, 0.0), (DISC, 1, 1.0)]
    want, groups = run_case(ctx, cols, [0], fns, "big", res=res)
    assert 99_000 < groups <= 100_000
    out = ctx.group_ordered(res, [0], fns)
    got = out.to_columns()
    k, v = ColumnExpression("k", 0, I64), ColumnExpression("v", 1, D)
    grouped = E.filter_groupby(ctx, batch, None, [ctx.compile(k)], [ctx.compile(v), ctx.compile(v)], [int(AF.MIN), int(AF.MAX)])
    g = grouped.to_columns()
    order = np.argsort(g[0].data, kind="stable")                     # insertion order -> ascending keys
    assert np.array_equal(g[0].data[order], got[0].data)
    for gb, mine in ((g[1], got[5]), (g[2], got[6])):
        gv = gb.valid[order] if gb.valid is not None else np.ones(groups, dtype=bool)
        mv = mine.valid if mine.valid is not None else np.ones(groups, dtype=bool)
        assert np.array_equal(gv, mv) and np.array_equal(gb.data[order][gv], mine.data[gv])
    win = ctx.window(res, [0], [(1, False)], [(N.WIN_DENSE_RANK,), (N.WIN_COUNT, 1)])
    w = win.to_columns()
    last = np.append(w[0].data[1:] != w[0].data[:-1], True)         # last row of every partition
    nulls = w[3].data[last] < np.diff(np.append(-1, np.nonzero(last)[0]))   # the NULL run in front is a peer group of its own
    assert np.array_equal(w[2].data[last] - nulls, got[1].data.astype(np.int64))
    win.free(); grouped.free(); out.free(); res.free(); batch.free()


# ---- DISTINCT --------------------------------------------------------------------------------------------------------------------
def test_select_distinct_over_two_key_columns(gpu_ctx):
    rng = np.random.default_rng(70)
    n = 5003
    cols = [Column(S, rng.integers(0, len(STRINGS), n).astype(np.int32), rng.random(n) > 0.1, STRINGS),
            Column(I32, rng.integers(-4, 4, n).astype(np.int32), rng.random(n) > 0.2), Column(D, rng.normal(0, 1, n))]
    want, groups = run_case(gpu_ctx, cols, [0, 1], [], "distinct")
    tuples = {(a if va else None, b if vb else None) for a, va, b, vb in zip(cols[0].data, cols[0].valid, cols[1].data, cols[1].valid)}
    assert groups == len(tuples) and len(want) == 2


# ---- the operator among the others ------------------------------------------------------------------------------------------------
def test_into_order_by_to_host_and_a_having_filter(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(71)
    n = 3000
    cols = [Column(I32, rng.integers(0, 40, n).astype(np.int32)), Column(D, rng.integers(-50, 50, n) / 2.0, rng.random(n) > 0.1)]
    batch, res = build(ctx, cols)
    fns = [E.MEDIAN(1), (CD, 1)]
    want, groups = ordered_reference(cols, [False, True], [0], fns)
    out = ctx.group_ordered(res, [0], fns)
    by_median = ctx.order_by_keys(out, [(1, True), (0, False)])
    assert by_median.count == groups
    med = by_median.column_to_host(1)
    assert np.all(np.diff(med.data) <= 0)
    host = out.to_host().wait()
    assert host.count == groups and np.array_equal(host.column(1).data, want[1].data)
    gbatch = out.as_batch()
    assert gbatch.nrows == groups and gbatch.ncols == 3
    median = ColumnExpression("median", 1, D)
    having = FunctionExpression(Function.CMP_GT, [median, NumericLiteralExpression(0.0)], B)
    kept = E.filter_project(ctx, gbatch, ctx.compile(having), [ctx.compile(ColumnExpression("k", 0, I32)), ctx.compile(median)])
    keep = want[1].valid & (want[1].data > 0.0)
    assert 0 < kept.count == int(keep.sum()) < groups
    assert np.array_equal(kept.column_to_host(0).data, want[0].data[keep]) and np.array_equal(kept.column_to_host(1).data, want[1].data[keep])
    kept.free(); gbatch.free(); host.free(); by_median.free(); out.free(); res.free(); batch.free()


def test_over_a_join_result(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(72)
    np_, nb = 4001, 37
    pcols = [Column(I32, rng.integers(0, 50, np_).astype(np.int32)), Column(D, rng.integers(-9, 9, np_) / 2.0, rng.random(np_) > 0.1)]
    bcols = [Column(I32, np.arange(nb, dtype=np.int32)), Column(S, (np.arange(nb) % len(STRINGS)).astype(np.int32), None, STRINGS)]
    pbatch, pres = build(ctx, pcols)
    bbatch, bres = build(ctx, bcols)
    table = ctx.join_build(bres, [0])
    joined = table.probe(pres, [0], N.JOIN_LEFT, [0, 1], [1])
    jcols = joined.to_columns()
    assert joined.count == np_
    run_case(ctx, jcols, [2], all_four(1) + [(MODE, 0)], "over a join", res=joined)     # the group key is NULL for unmatched rows
    table.free(); joined.free(); pres.free(); bres.free(); pbatch.free(); bbatch.free()


def test_operator_on_a_gpu_source_matches_its_host_branch(gpu_ctx):
    from queryengine_amd import ColumnarTable, Field, Schema
    from queryengine_amd.operators import GpuFilterProjectOperator, OrderedAggregateOperator, map as op_map
    from test_ordered_cpu import Rows, assert_rows
    rng = np.random.default_rng(73)
    n = 300
    cols = [Column(S, rng.integers(0, 4, n).astype(np.int32), rng.random(n) > 0.1, STRINGS), Column(D, rng.integers(-9, 9, n) / 4.0, rng.random(n) > 0.2)]
    table = ColumnarTable(Schema([Field("k", S), Field("v", D)]), cols)
    exprs = [ColumnExpression("k", 0, S), ColumnExpression("v", 1, D)]
    fns = all_four(1, 0.25) + [(MODE, 0)]
    dev = op_map(OrderedAggregateOperator(GpuFilterProjectOperator(gpu_ctx, table.getScanOperator(["k", "v"]), None, exprs), [0], fns), list)
    host = op_map(OrderedAggregateOperator(Rows([[c.value(i) for c in cols] for i in range(n)]), [0], fns), list)
    assert_rows(dev, host)


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_on_every_run_and_on_a_fresh_context(gpu_ctx):
    rng = np.random.default_rng(74)
    n = 3 * T + 5
    cols = [Column(I32, rng.integers(0, 7, n).astype(np.int32), rng.random(n) > 0.1), Column(D, rng.normal(0, 1, n).round(1), rng.random(n) > 0.1),
            Column(S, rng.integers(0, len(STRINGS), n).astype(np.int32), rng.random(n) > 0.1, STRINGS)]
    fns = all_four(1, 1 / 3) + all_four(2, 0.5, cont=False)

    def run(ctx):
        batch, res = build(ctx, cols)
        out = ctx.group_ordered(res, [0], fns)
        data = column_bytes(out)
        out.free(); res.free(); batch.free()
        return data

    first = run(gpu_ctx)
    assert run(gpu_ctx) == first
    other = E.Context(device=0)
    try:
        assert run(other) == first
    finally:
        other.close()


# ---- zero rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group_by", [[0], []], ids=["group-columns", "no-group-columns"])
def test_zero_input_rows(gpu_ctx, group_by):
    cols = [Column(S, np.zeros(0, dtype=np.int32), None, STRINGS), Column(D, np.zeros(0)), Column(B, np.zeros(0, dtype=bool))]
    fns = all_four(1) + all_four(0, cont=False) + [(MODE, 2)]
    want, groups = run_case(gpu_ctx, cols, group_by, fns, "zero rows")
    assert groups == (0 if group_by else 1) and len(want) == len(group_by) + len(fns)
    if not group_by:
        assert want[0].data[0] == 0.0 and want[0].valid[0] and not any(w.valid[0] for w in want[1:4])


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(gpu_ctx):
    rng = np.random.default_rng(75)
    n = 100
    cols = [Column(I32, rng.integers(0, 5, n).astype(np.int32)), Column(D, rng.normal(0, 1, n)), Column(S, rng.integers(0, 3, n).astype(np.int32), None, STRINGS),
            Column(B, rng.random(n) > 0.5)]
    batch, res = build(gpu_ctx, cols)
    lib = gpu_ctx._lib

    def call(group=(0,), fns=((CONT, 1, 0.5),), ngroup=None, nfn=None, null=(), ctx=gpu_ctx):
        g = (C.c_int32 * 16)(*group)
        f = (N.OrderedAgg * 32)(*[N.OrderedAgg(*x) for x in fns])
        out = C.c_void_p(0xdead)
        st = lib.qe_result_group_ordered(None if "ctx" in null else ctx.handle, None if "result" in null else res.handle,
                                         None if "group" in null else g, len(group) if ngroup is None else ngroup,
                                         None if "fns" in null else f, len(fns) if nfn is None else nfn, None if "out" in null else C.byref(out))
        if "out" not in null:
            if st != N.OK:
                assert out.value is None, "*out must be NULL after an error"
            else:
                lib.qe_result_free(ctx.handle, out)
        return st

    assert call() == N.OK
    for null in ("ctx", "result", "group", "fns", "out"):
        assert call(null=(null,)) == INVALID_ARG, null
    assert call(ngroup=-1) == INVALID_ARG and call(group=(0,) * 8) == INVALID_ARG and call(group=(0,) * 7) == N.OK
    assert call(nfn=-1) == INVALID_ARG and call(fns=((CD, 1, 0.0),) * 17) == INVALID_ARG and call(fns=((CD, 1, 0.0),) * 16) == N.OK
    assert call(group=(), fns=()) == INVALID_ARG                                           # both zero
    assert call(fns=()) == N.OK and call(group=()) == N.OK
    assert call(group=(4,)) == INVALID_ARG and call(group=(-1,)) == INVALID_ARG            # columns out of range
    assert call(fns=((CD, 4, 0.0),)) == INVALID_ARG and call(fns=((MODE, -1, 0.0),)) == INVALID_ARG
    assert call(fns=((4, 1, 0.0),)) == INVALID_ARG and call(fns=((-1, 1, 0.0),)) == INVALID_ARG   # unknown fn
    assert call(fns=((CONT, 2, 0.5),)) == INVALID_ARG and call(fns=((CONT, 3, 0.5),)) == INVALID_ARG   # STRING, BOOLEAN
    assert call(fns=((DISC, 2, 0.5),)) == N.OK and call(fns=((DISC, 3, 0.5),)) == N.OK
    for fn in (CONT, DISC):
        for q in (NAN, -0.001, 1.001, INF):
            assert call(fns=((fn, 1, q),)) == INVALID_ARG, (fn, q)
        assert call(fns=((fn, 1, 0.0),)) == N.OK and call(fns=((fn, 1, 1.0),)) == N.OK
    assert call(fns=((MODE, 1, NAN), (CD, 1, 7.0))) == N.OK                                # the fraction is not theirs
    planning = E.Context(device=None)
    try:
        assert call(ctx=planning) == HIP
        assert call(ctx=planning, group=(9,)) == INVALID_ARG
    finally:
        planning.close()
    run_case(gpu_ctx, cols, [0], all_four(1), "after the errors", res=res)                 # the context still works
    res.free(); batch.free()
