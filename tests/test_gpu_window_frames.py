"""qe_result_window_frames on the device: sliding and whole-partition frames, FIRST_VALUE / LAST_VALUE.

The expectation is tests/window_frames_reference.py (proved equal to the host branch of ``WindowOperator`` in
tests/test_window_frames_cpu.py); every output column is compared in full -- type, nullability, dictionary, validity, values by
bits.  Wherever sums are compared by bits the input is integer valued (multiples of 0.5, far below 2^53), so every order of
addition gives the same bits; fractional input is checked against ``math.fsum`` of the frame under the bound the header states,
with c and sum|x| of the FRAME.  Sizes are those where the kernels change behaviour: word (64), wave (512) and tile (2048)
edges for the frame width and for the partition edges, and one trip of the tile-aggregate scan (2 097 152 rows)."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from helpers import Fn, col, fn, num
from queryengine_amd import Column, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N

from test_gpu_window import STRINGS, build, exact_values, make_key
from window_frames_reference import frames_reference
from window_reference import T, TRIP, assert_window_output

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
UNB = N.FRAME_UNBOUNDED
INVALID_ARG, HIP = 1, 3
BIG = TRIP * T + 321
SEAM_N = 3 * T + 37
SEAM_LENGTHS = [1, 2, 63, 64, 65, 512, 513, 2048, 2049]


def run_frames(ctx, cols, part, order, fns, what, mode="exact"):
    """One call through ctx.window (qe_result_window_frames as soon as an entry names a frame) against the reference."""
    batch, res = build(ctx, cols)
    try:
        nullable = [bool(res.view(c).nullable) for c in range(res.ncols)]
        want, details = frames_reference(cols, nullable, part, order, fns, mode)
        out = ctx.window(res, part, order, fns)
        try:
            assert out.count == len(cols[0])
            assert_window_output(out, want, what)
            stats = ctx.last_window_stats()
            assert stats["rows"] == len(cols[0]) and stats["tiles"] == (len(cols[0]) + T - 1) // T, (what, stats)
        finally:
            out.free()
    finally:
        res.free(); batch.free()
    return want, details


def seven(column, p, f, first_col=None):
    first_col = column if first_col is None else first_col
    return [(N.WIN_SUM, column, 0, p, f), (N.WIN_COUNT, column, 0, p, f), (N.WIN_MIN, column, 0, p, f), (N.WIN_MAX, column, 0, p, f),
            (N.WIN_AVG, column, 0, p, f), (N.WIN_FIRST_VALUE, first_col, 0, p, f), (N.WIN_LAST_VALUE, first_col, 0, p, f)]


def column_bytes(result):
    return [(c.data.tobytes(), None if c.valid is None else c.valid.tobytes()) for c in result.to_columns()]


# ---- the running frame through the new entry ------------------------------------------------------------------------------------
def test_running_frame_is_byte_identical_to_qe_result_window(gpu_ctx):
    rng = np.random.default_rng(51)
    n = 5000
    cols = [make_key(I32, rng, n, coarse=True), make_key(D, rng, n, coarse=True), exact_values(rng, n, 0.01),
            Column(I64, rng.integers(-2 ** 40, 2 ** 40, n), rng.random(n) > 0.1), Column(I32, rng.integers(-9, 9, n).astype(np.int32), rng.random(n) > 0.1),
            make_key(S, rng, n, coarse=True, null_share=0.2), Column(I64, np.arange(n, dtype=np.int64))]
    short = [(N.WIN_ROW_NUMBER,), (N.WIN_RANK,), (N.WIN_DENSE_RANK,), (N.WIN_LAG, 5, 1), (N.WIN_LEAD, 2, 3)]
    for column in (2, 3, 4):
        short += [(N.WIN_SUM, column), (N.WIN_COUNT, column), (N.WIN_MIN, column), (N.WIN_MAX, column), (N.WIN_AVG, column)]
    batch, res = build(gpu_ctx, cols)
    for lot in (short[:10], short[10:]):
        long = [E.window_frame_fn(f) for f in lot]
        assert all(f[3:] == ((UNB, 0) if N.WIN_SUM <= f[0] <= N.WIN_AVG else (0, 0)) for f in long)
        old, new = gpu_ctx.window(res, [0], [(1, False)], lot), gpu_ctx.window(res, [0], [(1, False)], long)
        assert old.ncols == new.ncols == len(cols) + len(lot)
        assert [(old.view(k).type, old.view(k).nullable) for k in range(old.ncols)] == [(new.view(k).type, new.view(k).nullable) for k in range(new.ncols)]
        assert column_bytes(old) == column_bytes(new)
        old.free(); new.free()
    res.free(); batch.free()


# ---- frame widths and partition edges across word, wave and tile edges ----------------------------------------------------------
def seam_columns(rng, n=SEAM_N):
    lengths = []
    while sum(lengths) < n:
        lengths.append(SEAM_LENGTHS[rng.integers(0, len(SEAM_LENGTHS))])
    pid = np.repeat(np.arange(len(lengths)), lengths)[:n].astype(np.int64)
    return [Column(I64, pid), exact_values(rng, n, 0.0, 0.15), Column(I64, np.arange(n, dtype=np.int64)),
            Column(I32, rng.integers(-99, 99, n).astype(np.int32), rng.random(n) > 0.2)]


WIDTHS = [1, 2, 3, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049]
SEAM_FRAMES = [((w - 1) // 2, w - 1 - (w - 1) // 2) for w in WIDTHS] + [(SEAM_N, SEAM_N), (0, 70), (70, 0), (0, 2048), (2048, 0), (UNB, 5), (5, UNB),
                                                                         (UNB, 600), (600, UNB), (UNB, UNB), (0, UNB)]


@pytest.mark.parametrize("frame", SEAM_FRAMES, ids=lambda fr: f"p{fr[0]}f{fr[1]}".replace("-1", "U"))
def test_frame_widths_across_word_wave_and_tile_edges(gpu_ctx, frame):
    rng = np.random.default_rng(52)
    cols = seam_columns(rng)
    assert len(cols[0]) % 64 != 0
    run_frames(gpu_ctx, cols, [0], [(2, False)], seven(1, *frame, first_col=3), f"frame {frame}")


@pytest.mark.parametrize("plen", [0, 1000], ids=["one-partition", "partitions-of-1000"])
def test_a_partition_that_spans_a_trip_of_the_tile_scan(gpu_ctx, plen):
    rng = np.random.default_rng(53)
    n = BIG
    pid = np.zeros(n, dtype=np.int64) if plen == 0 else (np.arange(n) // plen).astype(np.int64)
    cols = [Column(I64, pid), exact_values(rng, n, 0.0, 0.1), Column(I64, np.arange(n, dtype=np.int64))]
    fns = []
    for p, f in [(1024, 1024), (UNB, UNB), (3, 3), (UNB, 5), (7, UNB)]:
        fns += [(N.WIN_SUM, 1, 0, p, f), (N.WIN_MAX, 1, 0, p, f)]
    fns += [(N.WIN_COUNT, 1, 0, 1024, 1024), (N.WIN_FIRST_VALUE, 2, 0, UNB, UNB), (N.WIN_LAST_VALUE, 2, 0, UNB, UNB), (N.WIN_LAST_VALUE, 1, 0, 0, 1024)]
    run_frames(gpu_ctx, cols, [0], [(2, False)], fns, f"n {n}, partitions of {plen or n}")
    assert gpu_ctx.last_window_stats()["trips"] == 2


@pytest.mark.parametrize("case", ["n0", "n1", "single-rows", "no-keys"])
def test_degenerate_inputs(gpu_ctx, case):
    rng = np.random.default_rng(54)
    n = {"n0": 0, "n1": 1}.get(case, 777)
    cols = [Column(I64, np.arange(n, dtype=np.int64) if case == "single-rows" else rng.integers(0, 5, n)), exact_values(rng, n, 0.0, 0.2),
            Column(S, rng.integers(0, len(STRINGS), n).astype(np.int32), rng.random(n) > 0.3, STRINGS)]
    part, order = ([], []) if case == "no-keys" else ([0], [(1, True)])
    fns = seven(1, 2, 2, first_col=2) + seven(1, UNB, UNB, first_col=2) + [(N.WIN_ROW_NUMBER, 0, 0, 0, 0), (N.WIN_LAG, 2, 1, 0, 0)]
    want, _ = run_frames(gpu_ctx, cols, part, order, fns, case)
    assert len(want) == 3 + 16 and len(want[0].data) == n
    if case == "no-keys" and n:      # one partition in input order: the whole-partition COUNT is one number
        assert set(want[3 + 8].data) == {float(cols[1].valid.sum())}


# ---- numerics --------------------------------------------------------------------------------------------------------------------
def test_fractional_sums_are_within_the_bound_of_the_frame(gpu_ctx):
    """|got - fsum| <= gamma_c * sum|x| with c and sum|x| of the FRAME (gamma_c = c*u / (1 - c*u), u = 2^-53); AVG within
    gamma_(c+1) * sum|x| / c (+ 2^-1075): the header's any-order bounds, derived and not measured."""
    rng = np.random.default_rng(55)
    n = 2 * T + 451
    vals = Column(D, 10.0 ** rng.uniform(-8, 12, n) * rng.choice([-1.0, 1.0], n), rng.random(n) >= 0.1)
    cols = [Column(I32, np.sort(rng.integers(0, 3, n)).astype(np.int32)), vals, Column(I64, np.arange(n, dtype=np.int64))]
    frames = [(3, 3), (0, 10), (50, 50), (UNB, UNB), (UNB, 4), (4, UNB), (700, 700)]
    fns = [(f, 1, 0, p, q) for p, q in frames for f in (N.WIN_SUM, N.WIN_AVG)]
    batch, res = build(gpu_ctx, cols)
    want, details = frames_reference(cols, [False, True, False], [0], [], fns, "slices")
    out = gpu_ctx.window(res, [0], [], fns)
    u, worst = Fraction(1, 2 ** 53), 0.0
    for k, (fnk, d) in enumerate(zip(fns, details)):
        got = out.column_to_host(3 + k)
        gv = got.valid if got.valid is not None else np.ones(n, dtype=bool)
        assert np.array_equal(gv, d["count"] > 0), fnk
        avg = fnk[0] == N.WIN_AVG
        for j in np.nonzero(gv)[0]:
            c = int(d["count"][j])
            m = c + 1 if avg else c
            bound = m * u / (1 - m * u) * Fraction(float(d["abs"][j])) / (c if avg else 1) + (Fraction(1, 2 ** 1075) if avg else 0)
            err = abs(Fraction(float(got.data[j])) - Fraction(float(d["sum"][j])) / (c if avg else 1))
            assert err <= bound, (fnk, int(j), c, float(err), float(bound))
            worst = max(worst, float(err / bound) if bound else 0.0)
    print(f"fractional framed SUM / AVG: worst error / bound = {worst:.3g}")
    out.free(); res.free(); batch.free()


def test_special_values_leave_the_frame(gpu_ctx):
    nan, inf = float("nan"), float("inf")
    n = 300
    rng = np.random.default_rng(56)
    v = rng.integers(-40, 41, n).astype(np.float64)
    valid = np.ones(n, dtype=bool)
    v[50], v[120], v[200] = inf, -inf, nan
    valid[10:30] = False                     # frames that hold no valid value
    v[240:270] = -0.0                        # frames of only -0.0
    cols = [Column(I32, np.zeros(n, dtype=np.int32)), Column(D, v, valid), Column(I64, np.arange(n, dtype=np.int64))]
    for p, f in [(3, 3), (0, 10)]:
        fns = [(N.WIN_SUM, 1, 0, p, f), (N.WIN_AVG, 1, 0, p, f), (N.WIN_MIN, 1, 0, p, f), (N.WIN_MAX, 1, 0, p, f), (N.WIN_COUNT, 1, 0, p, f)]
        run_frames(gpu_ctx, cols, [0], [(2, False)], fns, f"special values, frame ({p}, {f})", mode="slices")
        batch, res = build(gpu_ctx, cols)
        out = gpu_ctx.window(res, [0], [(2, False)], fns)
        got = [out.column_to_host(3 + k) for k in range(5)]
        for j in range(n):
            lo, hi = max(0, j - p), min(n - 1, j + f)
            inside = [x for x in (50, 120, 200) if lo <= x <= hi]
            rows = [i for i in range(lo, hi + 1) if valid[i]]
            if not rows:
                assert not any(g.valid[j] for g in got[:4]) and got[4].data[j] == 0.0, j
                continue
            s, a = got[0].data[j], got[1].data[j]
            if inside:
                want = nan if 200 in inside or len(inside) > 1 else v[inside[0]]
                assert (s != s and a != a) if want != want else (s == want and a == want), (j, s, a, want)
            else:            # finite and exact again once the special value has left: no trace of it
                assert math.isfinite(s) and s == sum(v[i] for i in rows) and a == s / len(rows), (j, s)
            if all(240 <= i < 270 for i in rows):
                assert s == 0.0 and math.copysign(1.0, s) == 1.0, j
                assert math.copysign(1.0, got[2].data[j]) == -1.0 and math.copysign(1.0, got[3].data[j]) == -1.0, j
        out.free(); res.free(); batch.free()


# ---- FIRST_VALUE / LAST_VALUE ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
def test_first_and_last_value_over_every_layout_of_column(gpu_ctx, descending):
    rng = np.random.default_rng(57)
    n = T + 333
    cols = [make_key(I32, rng, n, coarse=True), Column(D, rng.permutation(n).astype(np.float64)), make_key(S, rng, n, coarse=True, null_share=0.3),
            make_key(B, rng, n, coarse=True, null_share=0.3), make_key(I32, rng, n, coarse=False, null_share=0.3), make_key(B, rng, n, coarse=True, null_share=0.0),
            Column(I64, np.arange(n, dtype=np.int64))]
    fns = []
    for column in (2, 3, 4, 5):
        fns += [(N.WIN_FIRST_VALUE, column, 0, 2, 0), (N.WIN_LAST_VALUE, column, 0, 0, 65), (N.WIN_LAST_VALUE, column, 0, UNB, UNB), (N.WIN_FIRST_VALUE, column, 0, UNB, 0)]
    want, _ = run_frames(gpu_ctx, cols, [0], [(1, descending)], fns, f"first / last value, descending {descending}")
    assert want[7].dictionary == STRINGS and want[7].nullable and not want[7 + 12].nullable and (~want[7].valid).any()
    # a whole-partition LAST_VALUE is the value of the partition's last sorted row
    pid, last = want[0], want[7 + 4 * 2 + 2]           # LAST_VALUE of column 4 over (UNBOUNDED, UNBOUNDED)
    key = np.where(pid.valid, pid.data.astype(np.int64), np.int64(-1000))      # NULL is one key value
    ends = np.nonzero(np.append(key[1:] != key[:-1], True))[0]
    owner = ends[np.searchsorted(ends, np.arange(n))]
    assert np.array_equal(last.valid, want[4].valid[owner]) and np.array_equal(last.data[last.valid], want[4].data[owner][last.valid])


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_on_every_run_and_every_context(gpu_ctx):
    rng = np.random.default_rng(58)
    n = 100_000
    cols = [Column(I32, np.sort(rng.integers(0, 4, n)).astype(np.int32)), Column(D, rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 9, n), rng.random(n) > 0.1),
            Column(I64, np.arange(n, dtype=np.int64))]
    fns = [(N.WIN_SUM, 1, 0, 3, 3), (N.WIN_SUM, 1, 0, 1500, 1500), (N.WIN_AVG, 1, 0, UNB, UNB), (N.WIN_SUM, 1, 0, 9, UNB)]

    def run(ctx):
        batch, res = build(ctx, cols)
        out = ctx.window(res, [0], [(2, True)], fns)
        got = column_bytes(out)
        out.free(); res.free(); batch.free()
        return got

    first = run(gpu_ctx)
    assert run(gpu_ctx) == first
    other = E.Context(device=0)
    try:
        assert run(other) == first
    finally:
        other.close()


# ---- the framed result among the other operators -------------------------------------------------------------------------------------
def test_a_moving_average_feeds_a_filter_and_an_order_by(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(59)
    n = 4001
    cols = [Column(I32, rng.integers(0, 7, n).astype(np.int32)), exact_values(rng, n, 0.0, 0.1), Column(I64, np.arange(n, dtype=np.int64))]
    fns = [(N.WIN_AVG, 1, 0, 3, 3), (N.WIN_MAX, 1, 0, UNB, UNB)]
    want, _ = frames_reference(cols, [False, True, False], [0], [(2, False)], fns, "exact")
    batch, res = build(ctx, cols)
    out = ctx.window(res, [0], [(2, False)], fns)
    wbatch = out.as_batch()
    assert wbatch.nrows == n and wbatch.ncols == 5
    avg = col("avg", 3, D)
    kept = E.filter_project(ctx, wbatch, ctx.compile(fn(Fn.CMP_GT, avg, num(25.0))), [ctx.compile(col("rid", 2, I64)), ctx.compile(avg)])
    keep = want[3].valid & (np.where(want[3].valid, want[3].data, 0.0) > 25.0)
    got = kept.to_columns()
    assert 0 < kept.count == int(keep.sum()) < n
    assert np.array_equal(got[0].data, want[2].data[keep]) and np.array_equal(got[1].data, want[3].data[keep])
    srt = ctx.order_by_keys(out, [(3, True), (2, False)])
    g = srt.to_columns()
    rank = np.where(want[3].valid, want[3].data, -np.inf)           # descending: NULL last
    order = np.lexsort([want[2].data, -rank])
    assert np.array_equal(g[2].data, want[2].data[order])
    srt.free(); kept.free(); wbatch.free(); out.free(); res.free(); batch.free()


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(gpu_ctx):
    rng = np.random.default_rng(60)
    cols = [make_key(I32, rng, 100, True), exact_values(rng, 100), make_key(S, rng, 100, True), make_key(B, rng, 100, True)]
    batch, res = build(gpu_ctx, cols)
    lib = gpu_ctx._lib

    def call(fns=((N.WIN_SUM, 1, 0, 1, 1),), nfn=None, null=(), ctx=gpu_ctx):
        p = (C.c_int32 * 16)(0)
        o = (N.SortKey * 16)(N.SortKey(1, 0))
        f = (N.WindowFrameFn * 32)(*[N.WindowFrameFn(*x) for x in fns])
        out = C.c_void_p(0xdead)
        st = lib.qe_result_window_frames(None if "ctx" in null else ctx.handle, None if "result" in null else res.handle, p, 1, o, 1,
                                         None if "fns" in null else f, len(fns) if nfn is None else nfn, None if "out" in null else C.byref(out))
        if "out" not in null:
            if st != N.OK:
                assert out.value is None, "*out must be NULL after an error"
            else:
                lib.qe_result_free(ctx.handle, out)
        return st

    assert call() == N.OK
    for null in ("ctx", "result", "fns", "out"):
        assert call(null=(null,)) == INVALID_ARG, null
    for bad in ((-2, 0), (0, -2), (2 ** 31, 0), (0, 2 ** 31), (-2 ** 40, 0)):
        assert call(fns=((N.WIN_SUM, 1, 0) + bad,)) == INVALID_ARG, bad
    assert call(fns=((N.WIN_SUM, 1, 0, 2 ** 31 - 1, 2 ** 31 - 1),)) == N.OK and call(fns=((N.WIN_MIN, 1, 0, UNB, UNB),)) == N.OK
    for f in (N.WIN_FIRST_VALUE, N.WIN_LAST_VALUE):
        assert call(fns=((f, 4, 0, 1, 1),)) == INVALID_ARG and call(fns=((f, -1, 0, 1, 1),)) == INVALID_ARG      # column out of range
        assert call(fns=((f, 2, 0, 1, 1),)) == N.OK and call(fns=((f, 3, 0, UNB, 0),)) == N.OK                   # STRING, BOOLEAN
    for f in (N.WIN_ROW_NUMBER, N.WIN_RANK, N.WIN_DENSE_RANK, N.WIN_LAG, N.WIN_LEAD):
        assert call(fns=((f, 1, 1, 0, 0),)) == N.OK
        for frame in ((1, 0), (0, 1), (UNB, 0), (UNB, UNB)):
            assert call(fns=((f, 1, 1) + frame,)) == INVALID_ARG, (f, frame)
    assert call(fns=((12, 1, 0, 0, 0),)) == INVALID_ARG and call(fns=((-1, 1, 0, 0, 0),)) == INVALID_ARG
    assert call(fns=((N.WIN_SUM, 2, 0, 1, 1),)) == INVALID_ARG and call(fns=((N.WIN_AVG, 3, 0, 1, 1),)) == INVALID_ARG   # STRING, BOOLEAN
    assert call(fns=((N.WIN_LAG, 1, -1, 0, 0),)) == INVALID_ARG
    assert call(nfn=0) == INVALID_ARG and call(fns=((N.WIN_SUM, 1, 0, 1, 1),) * 17) == INVALID_ARG
    # qe_result_window itself does not learn the new functions
    old = (N.WindowFn * 1)(N.WindowFn(N.WIN_FIRST_VALUE, 1, 0))
    out = C.c_void_p(0xdead)
    assert lib.qe_result_window(gpu_ctx.handle, res.handle, None, 0, None, 0, old, 1, C.byref(out)) == INVALID_ARG and out.value is None
    planning = E.Context(device=None)
    try:
        assert call(ctx=planning) == HIP
    finally:
        planning.close()
    out = gpu_ctx.window(res, [0], [(1, False)], [(N.WIN_SUM, 1, 0, 1, 1)])      # the context still works
    assert out.count == 100
    out.free(); res.free(); batch.free()
