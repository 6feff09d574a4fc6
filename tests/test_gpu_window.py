"""qe_result_window on the device: ranks, running aggregates, LAG / LEAD over a sorted result.

The expectation is tests/window_reference.py (numpy; proved equal to the host branch of ``WindowOperator`` in
tests/test_window_cpu.py).  Every output column is compared in full -- type, nullability, dictionary, validity, values by
bits -- and an INT64 row id among the input columns pins the order including the ties.  Wherever a running SUM / AVG is
compared by bits its input is integer valued (multiples of 0.5, far below 2^53, plus NaN, the infinities and -0.0), so
every order of addition gives the same bits; fractional input is checked against the exact prefix sums under the bound the
header states.  T (rows of a scan tile) and the tiles one trip of the tile-aggregate scan covers are native.WIN_TILE_ROWS and
native.WIN_TRIP_TILES; the stats of the call confirm them.

One error of the contract has no test: a STRING key without a dictionary cannot be built through the ABI (every way to make
a STRING column demands one)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from queryengine_amd import AggregationFunction as AF
from queryengine_amd import Column, ColumnExpression, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N

from window_reference import T, TRIP, assert_window_output, window_reference

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
INVALID_ARG = 1
STRINGS = ["b", "a", "", "B", "～", "\U0001F600", "aa", "Zü", "zz", "a "]
DOUBLES = np.array([0.0, -0.0, 1.5, -1.5, float("nan"), float("inf"), -float("inf"), 1e300, -1e-300, 3.0])
INT64S = np.array([0, -1, 1, 2 ** 63 - 1, -(2 ** 63), 2 ** 53 + 1, 2 ** 63 - 2], dtype=np.int64)
SPECIALS = np.array([float("nan"), float("inf"), -float("inf"), -0.0])
BIG = TRIP * T + 321      # 321 rows more than one trip of the tile-aggregate scan covers


def make_key(t, rng, n, coarse, null_share=0.05):
    """A key column of type t with the special-value pools of the ORDER BY tests; coarse = tens of distinct values."""
    valid = rng.random(n) >= null_share if null_share > 0 else None
    if t == D:
        data = DOUBLES[rng.integers(0, len(DOUBLES), n)]
        if not coarse:
            data = np.where(rng.random(n) < 0.5, data, rng.normal(0, 1e3, n))
        return Column(D, data, valid)
    if t == I64:
        data = INT64S[rng.integers(0, len(INT64S), n)]
        return Column(I64, data if coarse else np.where(rng.random(n) < 0.3, data, rng.integers(-5000, 5000, n)), valid)
    if t == I32:
        return Column(I32, (rng.integers(-8, 8, n) if coarse else rng.integers(-2 ** 31, 2 ** 31 - 1, n)).astype(np.int32), valid)
    if t == S:
        return Column(S, rng.integers(0, len(STRINGS), n).astype(np.int32), valid, STRINGS)
    return Column(B, rng.random(n) > 0.5, valid)


def exact_values(rng, n, special_share=0.0, null_share=0.1):
    """A DOUBLE column whose running sums are exact in every order: multiples of 0.5 in [-500, 500], NULLs, and (on request)
    NaN, +-inf and -0.0."""
    data = rng.integers(-1000, 1001, n) / 2.0
    if special_share > 0:
        pick = rng.random(n) < special_share
        data = np.where(pick, SPECIALS[rng.integers(0, len(SPECIALS), n)], data)
    return Column(D, data, rng.random(n) >= null_share if null_share > 0 else None)


def build(ctx, cols):
    """filter_project over an identity projection: a result that holds exactly `cols`."""
    batch = E.DeviceBatch.from_columns(ctx, cols)
    projs = [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)]
    return batch, E.filter_project(ctx, batch, None, projs)


def run_case(ctx, cols, part, order, fns, what, res=None):
    """One qe_result_window against the reference; returns the stats of the call."""
    batch = None
    if res is None:
        batch, res = build(ctx, cols)
    try:
        nullable = [bool(res.view(c).nullable) for c in range(res.ncols)]
        want, _, nparts = window_reference(cols, nullable, part, order, fns)
        out = ctx.window(res, part, order, fns)
        try:
            stats = ctx.last_window_stats()
            assert out.count == len(cols[0])
            assert_window_output(out, want, what)
            assert stats["rows"] == len(cols[0]) and stats["partitions"] == nparts, (what, stats, nparts)
            assert stats["tiles"] == (len(cols[0]) + T - 1) // T and stats["trips"] == (stats["tiles"] + TRIP - 1) // TRIP, (what, stats)
        finally:
            out.free()
    finally:
        if batch is not None:
            res.free(); batch.free()
    return stats


def standard_columns(rng, n, ptype=I32, special_share=0.01):
    """(partition key, order key with ties, exact DOUBLE values, nullable STRING payload, nullable BOOLEAN payload, row id)"""
    return [make_key(ptype, rng, n, coarse=True), make_key(D, rng, n, coarse=True), exact_values(rng, n, special_share),
            make_key(S, rng, n, coarse=True, null_share=0.2), make_key(B, rng, n, coarse=True, null_share=0.2),
            Column(I64, np.arange(n, dtype=np.int64))]


ALL_TEN = [(N.WIN_ROW_NUMBER,), (N.WIN_RANK,), (N.WIN_DENSE_RANK,), (N.WIN_SUM, 2), (N.WIN_COUNT, 3), (N.WIN_MIN, 2), (N.WIN_MAX, 2),
           (N.WIN_AVG, 2), (N.WIN_LAG, 3, 1), (N.WIN_LEAD, 4, 2)]


@pytest.mark.parametrize("fn", ALL_TEN + [ALL_TEN], ids=lambda f: "all" if isinstance(f, list) else f"fn{f[0]}")
def test_each_function_alone_and_all_ten_together(gpu_ctx, fn):
    rng = np.random.default_rng(21)
    cols = standard_columns(rng, 6007)
    run_case(gpu_ctx, cols, [0], [(1, False)], fn if isinstance(fn, list) else [fn], "functions")


@pytest.mark.parametrize("ptype", [D, I64, I32, B, S, (S, D)], ids=lambda t: t.name if isinstance(t, DataType) else "two-columns")
def test_partition_key_types(gpu_ctx, ptype):
    rng = np.random.default_rng(22)
    n = 5003
    if isinstance(ptype, tuple):
        cols = standard_columns(rng, n, ptype[0])
        cols.append(make_key(ptype[1], rng, n, coarse=True))
        run_case(gpu_ctx, cols, [0, 6], [(1, True)], ALL_TEN, "two partition columns")
    else:
        cols = standard_columns(rng, n, ptype)
        run_case(gpu_ctx, cols, [0], [(1, True), (5, True)], ALL_TEN, f"partition by {ptype.name}")


@pytest.mark.parametrize("part,order", [([], [(1, False)]), ([0], []), ([], [])], ids=["npart0", "norder0", "both0"])
def test_without_partition_or_order_keys(gpu_ctx, part, order):
    rng = np.random.default_rng(23)
    cols = standard_columns(rng, 2 * T + 77, special_share=0.0005)
    run_case(gpu_ctx, cols, part, order, ALL_TEN, f"part {part} order {order}")


# ---- sizes at the scan's seams ---------------------------------------------------------------------------------------------
def layout_starts(rng, n, layout):
    """bool per row: the row starts a partition."""
    start = np.zeros(n, dtype=bool)
    if n == 0:
        return start
    start[0] = True
    if layout == "one":
        return start
    if layout == "each":
        start[:] = True
        return start
    # partitions of random length 1 .. 3T, and starts forced onto lane 0, lane 63, the first and the last row of a tile
    pos = np.cumsum(rng.integers(1, 3 * T + 1, max(2, n // T + 2)))
    start[pos[pos < n]] = True
    ntiles = (n + T - 1) // T
    for tile in sorted({0, 1, ntiles // 2, ntiles - 2, ntiles - 1} & set(range(ntiles))):
        for p in (tile * T, tile * T + T - 1, tile * T + 64 * 5, tile * T + 64 * 9 + 63, tile * T + 512, tile * T + 511):
            if p < n:
                start[p] = True
    return start


SEAM_FNS = [(N.WIN_ROW_NUMBER,), (N.WIN_RANK,), (N.WIN_DENSE_RANK,), (N.WIN_SUM, 1), (N.WIN_COUNT, 1), (N.WIN_MIN, 1), (N.WIN_MAX, 1),
            (N.WIN_AVG, 1), (N.WIN_LAG, 1, 1), (N.WIN_LEAD, 2, T)]


@pytest.mark.parametrize("layout", ["one", "each", "random"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, BIG])
def test_sizes_at_the_seams_of_the_scan(gpu_ctx, n, layout):
    rng = np.random.default_rng(3000 + n % 1000 + len(layout))
    start = layout_starts(rng, n, layout)
    # the rows arrive shuffled: partition id ascending and the position inside it (in pairs: ties) put them back
    shuffle = rng.permutation(n)
    pid = np.cumsum(start).astype(np.int64)
    pos = (np.arange(n) // 2).astype(np.float64)
    cols = [Column(I64, pid[shuffle]), exact_values(rng, n, 0.0, 0.15), Column(D, pos[shuffle]), Column(I64, shuffle.astype(np.int64))]
    stats = run_case(gpu_ctx, cols, [0], [(2, False)], SEAM_FNS, f"n {n} layout {layout}")
    if n == BIG:
        assert stats["trips"] >= 2 and stats["tiles"] == TRIP + 1
        assert stats["partitions"] == int(start.sum())


# ---- numerics ---------------------------------------------------------------------------------------------------------------
def test_fractional_sum_and_avg_are_within_the_stated_bound(gpu_ctx):
    """SUM within gamma_c * sum|x| of the exact prefix sum (c valid values so far, gamma_c = c*u / (1 - c*u), u = 2^-53), AVG
    within gamma_(c+1) * sum|x| / c (+ 2^-1075): the any-order bounds of the header, derived and not measured."""
    rng = np.random.default_rng(24)
    n = 4999
    mag = 10.0 ** rng.uniform(-8, 12, n)
    vals = Column(D, mag * rng.choice([-1.0, 1.0], n), rng.random(n) >= 0.1)
    pid = Column(I32, np.sort(rng.integers(0, 3, n)).astype(np.int32))
    cols = [pid, vals, Column(I64, np.arange(n, dtype=np.int64))]
    batch, res = build(gpu_ctx, cols)
    out = gpu_ctx.window(res, [0], [], [(N.WIN_SUM, 1), (N.WIN_AVG, 1)])
    got_sum, got_avg = out.column_to_host(3), out.column_to_host(4)
    u = Fraction(1, 2 ** 53)
    exact, absum, c, worst = Fraction(0), Fraction(0), 0, 0.0
    valid = vals.valid if vals.valid is not None else np.ones(n, dtype=bool)
    for j in range(n):
        if j == 0 or pid.data[j] != pid.data[j - 1]:
            exact, absum, c = Fraction(0), Fraction(0), 0
        if valid[j]:
            exact += Fraction(float(vals.data[j]))
            absum += abs(Fraction(float(vals.data[j])))
            c += 1
        if c == 0:
            assert got_sum.valid is not None and not got_sum.valid[j] and not got_avg.valid[j]
            continue
        assert (got_sum.valid is None or got_sum.valid[j]) and (got_avg.valid is None or got_avg.valid[j])
        gamma = c * u / (1 - c * u)
        err = abs(Fraction(float(got_sum.data[j])) - exact)
        assert err <= gamma * absum, (j, c, float(err), float(gamma * absum))
        gamma1 = (c + 1) * u / (1 - (c + 1) * u)
        aerr = abs(Fraction(float(got_avg.data[j])) - exact / c)
        assert aerr <= gamma1 * absum / c + Fraction(1, 2 ** 1075), (j, c, float(aerr))
        worst = max(worst, float(err / (gamma * absum)) if absum else 0.0)
    print(f"fractional running SUM: worst error / bound = {worst:.3g}")
    out.free(); res.free(); batch.free()


def test_special_values_in_the_value_column(gpu_ctx):
    nan, inf = float("nan"), float("inf")
    rows = [(1, None), (1, None), (1, 2.5), (1, None), (1, -0.5),
            (2, -0.0), (2, -0.0), (2, 0.0),
            (3, 1.0), (3, inf), (3, 2.0), (3, -inf), (3, 3.0),
            (4, 5.0), (4, nan), (4, 1.0)]
    cols = [Column.from_values(I32, [r[0] for r in rows]), Column.from_values(D, [r[1] for r in rows]),
            Column.from_values(S, ["s", None, "t", "s"] * 4)]
    fns = [(N.WIN_SUM, 1), (N.WIN_COUNT, 1), (N.WIN_MIN, 1), (N.WIN_MAX, 1), (N.WIN_AVG, 1), (N.WIN_COUNT, 2)]
    batch, res = build(gpu_ctx, cols)
    out = gpu_ctx.window(res, [0], [], fns)
    got = out.to_columns()
    sums = [got[3].value(i) for i in range(len(rows))]
    assert sums[:5] == [None, None, 2.5, 2.5, 2.0]
    assert [math.copysign(1.0, v) for v in sums[5:8]] == [1.0, 1.0, 1.0] and sums[5:8] == [0.0, 0.0, 0.0]     # only -0.0: +0.0
    assert sums[8:11] == [1.0, inf, inf] and all(v != v for v in sums[11:13])                                     # both infinities: NaN to the end
    assert sums[13] == 5.0 and all(v != v for v in sums[14:])
    mins, maxs = [got[5].value(i) for i in range(len(rows))], [got[6].value(i) for i in range(len(rows))]
    assert [math.copysign(1.0, v) for v in mins[5:8]] == [-1.0, -1.0, -1.0]                                       # -0.0 below +0.0
    assert [math.copysign(1.0, v) for v in maxs[5:8]] == [-1.0, -1.0, 1.0]
    assert mins[11] == -inf and maxs[11] == inf and all(v != v for v in mins[14:] + maxs[14:])                    # NaN wins
    assert [got[8].value(i) for i in range(len(rows))] == [1.0, 1.0, 2.0, 3.0, 4.0, 0.0, 1.0, 2.0, 1.0, 1.0, 2.0, 3.0, 4.0, 0.0, 1.0, 2.0]
    out.free(); res.free(); batch.free()
    run_case(gpu_ctx, cols, [0], [], fns, "special values")


@pytest.mark.parametrize("nullable", [True, False], ids=["nullable", "not-nullable"])
@pytest.mark.parametrize("t", [D, B, S], ids=lambda t: t.name)
def test_lag_and_lead_over_every_layout_of_column(gpu_ctx, t, nullable):
    rng = np.random.default_rng(25)
    n = 2 * T + 333
    start = layout_starts(rng, n, "random")
    start[rng.integers(0, n, 40)] = True
    cols = [Column(I64, np.cumsum(start).astype(np.int64)), make_key(t, rng, n, coarse=False, null_share=0.2 if nullable else 0.0),
            Column(I64, np.arange(n, dtype=np.int64))]
    fns = []
    for off in (0, 1, 64, T, n + 5):
        fns += [(N.WIN_LAG, 1, off), (N.WIN_LEAD, 1, off)]
    run_case(gpu_ctx, cols, [0], [], fns, f"lag / lead over {t.name}")
    run_case(gpu_ctx, cols, [], [], fns[:8], f"lag / lead over {t.name}, one partition")


def test_the_same_bytes_on_every_run_and_every_context(gpu_ctx):
    rng = np.random.default_rng(26)
    n = 5 * T + 123
    cols = [Column(I32, np.sort(rng.integers(0, 4, n)).astype(np.int32)), Column(D, rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 9, n), rng.random(n) > 0.1),
            Column(I64, np.arange(n, dtype=np.int64))]

    def run(ctx):
        batch, res = build(ctx, cols)
        out = ctx.window(res, [0], [(2, True)], [(N.WIN_SUM, 1), (N.WIN_AVG, 1)])
        got = []
        for c in out.to_columns():
            got.append((c.data.tobytes(), None if c.valid is None else c.valid.tobytes()))
        out.free(); res.free(); batch.free()
        return got

    first = run(gpu_ctx)
    assert run(gpu_ctx) == first
    other = E.Context(device=0)
    try:
        assert run(other) == first
    finally:
        other.close()


# ---- the operator among the others ----------------------------------------------------------------------------------------------
def test_over_a_join_result_and_into_a_group_by(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(27)
    np_, nb = 4001, 37
    pcols = [Column(I32, rng.integers(0, 50, np_).astype(np.int32)), exact_values(rng, np_), Column(I64, np.arange(np_, dtype=np.int64))]
    bcols = [Column(I32, np.arange(nb, dtype=np.int32)), Column(S, (np.arange(nb) % len(STRINGS)).astype(np.int32), None, STRINGS)]
    pbatch, pres = build(ctx, pcols)
    bbatch, bres = build(ctx, bcols)
    table = ctx.join_build(bres, [0])
    joined = table.probe(pres, [0], N.JOIN_INNER, [0, 1, 2], [1])
    jcols = joined.to_columns()
    assert 0 < joined.count < np_
    fns = [(N.WIN_ROW_NUMBER,), (N.WIN_SUM, 1), (N.WIN_LAG, 3, 1)]
    run_case(ctx, jcols, [3], [(2, True)], fns, "over a join", res=joined)
    # the windowed result goes on into a GROUP BY through as_batch(): the last ROW_NUMBER of a partition is its row count
    out = ctx.window(joined, [3], [(2, True)], fns)
    wbatch = out.as_batch()
    assert wbatch.nrows == joined.count and wbatch.ncols == 7
    key, rn = ColumnExpression("tag", 3, S), ColumnExpression("rn", 4, I64)
    grouped = E.filter_groupby(ctx, wbatch, None, [ctx.compile(key)], [ctx.compile(rn), ctx.compile(rn)], [int(AF.MAX), int(AF.COUNT)])
    g = grouped.to_columns()
    assert grouped.count == len(set(jcols[3].to_list()))
    assert np.array_equal(g[1].data, g[2].data)
    grouped.free(); wbatch.free(); out.free()
    table.free(); joined.free(); pres.free(); bres.free(); pbatch.free(); bbatch.free()


def test_window_operator_on_a_gpu_source_matches_its_host_branch(gpu_ctx):
    from queryengine_amd import Field, Schema, ColumnarTable
    from queryengine_amd.operators import GpuFilterProjectOperator, Operator, WindowOperator, map as op_map
    rng = np.random.default_rng(28)
    n = 300
    cols = [make_key(S, rng, n, coarse=True), make_key(I32, rng, n, coarse=True), exact_values(rng, n, 0.02)]
    table = ColumnarTable(Schema([Field("p", S), Field("o", I32), Field("v", D)]), cols)
    exprs = [ColumnExpression("p", 0, S), ColumnExpression("o", 1, I32), ColumnExpression("v", 2, D)]
    fns = [(N.WIN_RANK,), (N.WIN_SUM, 2), (N.WIN_COUNT, 2), (N.WIN_LEAD, 0, 1)]

    class Rows(Operator):
        def __init__(self, rows):
            self.rows, self.i = rows, None

        def open(self):
            self.i = 0

        def close(self):
            self.i = None

        def next(self):
            if self.i >= len(self.rows):
                return None
            self.i += 1
            return self.rows[self.i - 1]

    dev = op_map(WindowOperator(GpuFilterProjectOperator(gpu_ctx, table.getScanOperator(["p", "o", "v"]), None, exprs), [0], [(1, True)], fns), list)
    host = op_map(WindowOperator(Rows([[c.value(i) for c in cols] for i in range(n)]), [0], [(1, True)], fns), list)
    assert len(dev) == len(host) == n
    for a, b in zip(dev, host):
        assert len(a) == len(b) and all(x == y or (x != x and y != y) for x, y in zip(a, b)), (a, b)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(gpu_ctx):
    rng = np.random.default_rng(29)
    cols = [make_key(I32, rng, 100, True), exact_values(rng, 100), make_key(S, rng, 100, True), make_key(B, rng, 100, True)]
    batch, res = build(gpu_ctx, cols)
    lib = gpu_ctx._lib

    def call(part=(0,), order=((1, 0),), fns=((N.WIN_SUM, 1, 0),), npart=None, norder=None, nfn=None, null=()):
        p = (C.c_int32 * 16)(*part)
        o = (N.SortKey * 16)(*[N.SortKey(c, d) for c, d in order])
        f = (N.WindowFn * 32)(*[N.WindowFn(*x) for x in fns])
        out = C.c_void_p(0xdead)
        st = lib.qe_result_window(None if "ctx" in null else gpu_ctx.handle, None if "result" in null else res.handle,
                                  None if "part" in null else p, len(part) if npart is None else npart,
                                  None if "order" in null else o, len(order) if norder is None else norder,
                                  None if "fns" in null else f, len(fns) if nfn is None else nfn, None if "out" in null else C.byref(out))
        if "out" not in null:
            if st != N.OK:
                assert out.value is None, "*out must be NULL after an error"
            else:
                lib.qe_result_free(gpu_ctx.handle, out)
        return st

    assert call() == N.OK
    for null in ("result", "part", "order", "fns", "out"):
        assert call(null=(null,)) == INVALID_ARG, null
    assert call(npart=-1) == INVALID_ARG and call(norder=-1) == INVALID_ARG
    assert call(part=(0,) * 5, order=((1, 0),) * 4) == INVALID_ARG                       # npart + norder > 8
    assert call(part=(0,) * 4, order=((1, 0),) * 4) == N.OK
    assert call(nfn=0) == INVALID_ARG and call(fns=((N.WIN_ROW_NUMBER, 0, 0),) * 17) == INVALID_ARG
    assert call(fns=((N.WIN_ROW_NUMBER, 0, 0),) * 16) == N.OK
    assert call(part=(4,)) == INVALID_ARG and call(part=(-1,)) == INVALID_ARG            # columns out of range
    assert call(order=((4, 0),)) == INVALID_ARG and call(fns=((N.WIN_SUM, 4, 0),)) == INVALID_ARG
    assert call(fns=((N.WIN_LAG, -1, 0),)) == INVALID_ARG
    assert call(fns=((N.WIN_ROW_NUMBER, 99, 0),)) == N.OK                                # ignored by the ranks
    assert call(fns=((10, 1, 0),)) == INVALID_ARG and call(fns=((-1, 1, 0),)) == INVALID_ARG
    for fn in (N.WIN_SUM, N.WIN_MIN, N.WIN_MAX, N.WIN_AVG):
        assert call(fns=((fn, 2, 0),)) == INVALID_ARG and call(fns=((fn, 3, 0),)) == INVALID_ARG   # STRING, BOOLEAN
    assert call(fns=((N.WIN_COUNT, 2, 0),)) == N.OK and call(fns=((N.WIN_COUNT, 3, 0),)) == N.OK
    assert call(fns=((N.WIN_LAG, 1, -1),)) == INVALID_ARG and call(fns=((N.WIN_LEAD, 1, 2 ** 31),)) == INVALID_ARG
    assert call(fns=((N.WIN_LEAD, 1, 2 ** 31 - 1),)) == N.OK
    run_case(gpu_ctx, cols, [0], [(1, False)], [(N.WIN_SUM, 1)], "after the errors", res=res)      # the context still works
    res.free(); batch.free()
