"""Ordered-set aggregates per group without a GPU: the host branch of ``OrderedAggregateOperator`` against a hand-written
table, the numpy reference of the device tests (tests/ordered_reference.py) against that host branch value for value, and the
argument checks of the Python layer and of qe_result_group_ordered that need no device."""
import ctypes as C
import itertools
import struct

import numpy as np
import pytest

from queryengine_amd import Column, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N
from queryengine_amd.operators import Operator, OrderedAggregateOperator, map as op_map

from ordered_reference import ordered_reference

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
NAN, INF = float("nan"), float("inf")
CD, CONT, DISC, MODE = N.OSA_COUNT_DISTINCT, N.OSA_PERCENTILE_CONT, N.OSA_PERCENTILE_DISC, N.OSA_MODE
FRACTIONS = [0.0, 0.25, 1 / 3, 0.5, 2 / 3, 0.999, 1.0]
STRINGS = ["b", "a", "", "B", "～", "\U0001F600", "aa", "Zü", "zz", "a "]     # not in sorted order


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


def grouped(rows, group_by, functions):
    return op_map(OrderedAggregateOperator(Rows([list(r) for r in rows]), group_by, functions), lambda r: list(r))


def same(a, b):
    """NaN compares by "both NaN"; every other value by bits (so -0.0 is not 0.0, and an int is not a float)."""
    if isinstance(a, float) and isinstance(b, float) and a != a and b != b:
        return True
    if isinstance(a, float) and isinstance(b, float):
        return struct.pack("<d", a) == struct.pack("<d", b)
    return type(a) is type(b) and a == b


def assert_rows(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and all(same(x, y) for x, y in zip(g, w)), f"row {i}: got {g}, want {w}"


def reference_rows(cols, group_by, functions):
    """The reference's expected columns as boxed rows, COUNT_DISTINCT as the int the operator returns."""
    want, G = ordered_reference(cols, [c.valid is not None for c in cols], group_by, functions)
    boxed = [Column(w.type, w.data, w.valid, w.dictionary) for w in want]
    rows = [[c.value(i) for c in boxed] for i in range(G)]
    for r in rows:
        for k, f in enumerate(functions):
            if f[0] == CD:
                r[len(group_by) + k] = int(r[len(group_by) + k])
    return rows


# ---- expectations typed out ------------------------------------------------------------------------------------------------------
# (group key, DOUBLE value, STRING value)
TABLE = [("y", 4.0, "q"), ("x", 1.0, "b"), (None, 7.0, None), ("x", None, "a"), ("y", 2.0, "q"), ("x", 3.0, "b"), ("y", 2.0, "p"),
         ("x", 1.0, "a"), ("z", None, None), ("y", 10.0, "p"), ("x", 6.0, "c")]


def test_a_table_with_the_expectations_typed_out():
    fns = [(CD, 1), (CONT, 1, 0.5), (DISC, 1, 0.5), (MODE, 1), (CONT, 1, 0.25), (DISC, 1, 1.0), (CD, 2), (MODE, 2), (DISC, 2, 0.0)]
    got = grouped(TABLE, [0], fns)
    # NULL key first.  x: values 1 1 3 6, strings a a b b c.  y: values 2 2 4 10, strings p p q q.  z: nothing.
    want = [[None, 1, 7.0, 7.0, 7.0, 7.0, 7.0, 0, None, None],
            ["x", 3, 2.0, 1.0, 1.0, 1.0, 6.0, 3, "a", "a"],       # median (1 + 3) / 2; disc(0.5): k = ceil(2) - 1 = 1; cont(0.25): h = 0.75 -> 1 + 0 * 0.75
            ["y", 3, 3.0, 2.0, 2.0, 2.0, 10.0, 2, "p", "p"],      # cont(0.25): v[0] and v[1] have the same bits
            ["z", 0, None, None, None, None, None, 0, None, None]]
    assert_rows(got, want)
    assert_rows(got, reference_rows(columns_of(TABLE), [0], fns))


def columns_of(table):
    keys = sorted({r[0] for r in table if r[0] is not None}, reverse=True)
    strs = sorted({r[2] for r in table if r[2] is not None}, reverse=True)
    return [Column(S, np.array([keys.index(r[0]) if r[0] is not None else 0 for r in table], dtype=np.int32),
                   np.array([r[0] is not None for r in table]), keys),
            Column(D, np.array([r[1] if r[1] is not None else 0.0 for r in table]), np.array([r[1] is not None for r in table])),
            Column(S, np.array([strs.index(r[2]) if r[2] is not None else 0 for r in table], dtype=np.int32),
                   np.array([r[2] is not None for r in table]), strs)]


def test_interpolation_is_the_formula_in_its_order():
    rows = [(0, 0.1), (0, 0.7), (0, 0.2)]
    got = grouped(rows, [0], [(CONT, 1, 1 / 3), (CONT, 1, 0.999)])
    h = (1 / 3) * 2.0
    frac = h - 0.0
    assert same(got[0][1], 0.1 + (0.2 - 0.1) * frac)
    h = 0.999 * 2.0
    assert same(got[0][2], 0.2 + (0.7 - 0.2) * (h - 1.0))


def test_infinities_nan_and_signed_zeros():
    rows = [(0, INF), (0, INF), (1, -INF), (1, INF), (2, 1.0), (2, NAN), (3, -0.0), (3, 0.0), (3, NAN), (3, NAN)]
    got = grouped(rows, [0], [(CONT, 1, 0.5), (CD, 1), (MODE, 1), (DISC, 1, 0.0), (DISC, 1, 1.0)])
    assert_rows(got, [[0, INF, 1, INF, INF, INF],                   # the same bits: no inf - inf
                      [1, NAN, 2, -INF, -INF, INF],                 # -inf + (inf - -inf) * 0.5 = -inf + inf
                      [2, NAN, 2, 1.0, 1.0, NAN],
                      [3, NAN, 3, NAN, -0.0, NAN]])                 # -0.0 < 0.0 < NaN = NaN: three values, h = 1.5 reaches a NaN


# ---- the numpy reference equals the host branch ---------------------------------------------------------------------------------
POOLS = {D: [NAN, -0.0, 0.0, INF, -INF, 1.5, -2.25, 1e300, 0.1, 0.7],
         I64: [2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, -(2 ** 53) - 1, -(2 ** 53), 0, 7, -7, 2 ** 63 - 1, -(2 ** 63)],
         I32: [0, 1, -1, 2 ** 31 - 1, -(2 ** 31), 5, 5, 9], B: [False, True], S: list(range(len(STRINGS)))}
NPTYPE = {D: np.float64, I64: np.int64, I32: np.int32, B: bool, S: np.int32}


def group_column(t, rng, lengths, nulls):
    """One argument column: group g holds lengths[g] valid values drawn from the type's pool and nulls[g] NULLs, shuffled."""
    data, valid = [], []
    for c, z in zip(lengths, nulls):
        pool = POOLS[t]
        data += [pool[i] for i in rng.integers(0, len(pool), c)] + [pool[0]] * z
        valid += [True] * c + [False] * z
    return np.array(data, dtype=NPTYPE[t]), np.array(valid, dtype=bool)


@pytest.mark.parametrize("t", [D, I64, I32, B, S], ids=lambda t: t.name)
def test_the_numpy_reference_equals_the_host_branch(t):
    """Groups of 0..5 valid values with 0..2 NULLs, every fraction, every function the type takes; special values in the pools."""
    rng = np.random.default_rng(300 + int(t))
    shapes = [(c, z) for c in range(6) for z in range(3) if c + z > 0] * 3
    lengths, nulls = [s[0] for s in shapes], [s[1] for s in shapes]
    gid = np.repeat(np.arange(len(shapes)), [c + z for c, z in shapes]).astype(np.int64)
    data, valid = group_column(t, rng, lengths, nulls)
    shuffle = rng.permutation(len(gid))
    cols = [Column(I64, gid[shuffle]), Column(t, data[shuffle], valid[shuffle], STRINGS if t == S else None)]
    rows = [[c.value(i) for c in cols] for i in range(len(gid))]
    fns = [(CD, 1), (MODE, 1)] + [(DISC, 1, q) for q in FRACTIONS] + ([(CONT, 1, q) for q in FRACTIONS] if t in (D, I64, I32) else [])
    assert_rows(grouped(rows, [0], fns), reference_rows(cols, [0], fns))
    assert_rows(grouped(rows, [], fns), reference_rows(cols, [], fns))           # one group
    assert_rows(grouped(rows, [1], fns[:3]), reference_rows(cols, [1], fns[:3]))  # the argument as its own group key, NULL included


def test_several_group_columns_distinct_and_empty_input():
    rng = np.random.default_rng(7)
    n = 400
    cols = [Column(S, rng.integers(0, len(STRINGS), n).astype(np.int32), rng.random(n) > 0.1, STRINGS),
            Column(D, np.array(POOLS[D])[rng.integers(0, 5, n)], rng.random(n) > 0.1),
            Column(I32, rng.integers(-3, 3, n).astype(np.int32), rng.random(n) > 0.2), Column(B, rng.random(n) > 0.5, rng.random(n) > 0.2)]
    rows = [[c.value(i) for c in cols] for i in range(n)]
    fns = [(CD, 2), (E.MEDIAN(2)), (MODE, 3), (DISC, 3, 0.5), (CD, 3), (MODE, 0)]
    assert_rows(grouped(rows, [0, 1], fns), reference_rows(cols, [0, 1], fns))
    distinct = grouped(rows, [0, 2], [])                                          # SELECT DISTINCT
    assert_rows(distinct, reference_rows(cols, [0, 2], []))
    assert len(distinct) == len({(r[0], r[2]) for r in rows})
    empty = [Column(c.type, c.data[:0], None, c.dictionary) for c in cols]
    assert grouped([], [0], fns) == [] and reference_rows(empty, [0], fns) == []
    assert_rows(grouped([], [], fns), [[0, None, None, None, 0, None]])          # the one group of nothing
    assert_rows(reference_rows(empty, [], fns), [[0, None, None, None, 0, None]])


def test_int64_is_sorted_before_it_is_converted():
    big = 2 ** 53
    rows = [(0, big + 1), (0, big), (0, big + 2), (0, big + 1)]
    got = grouped(rows, [0], [(DISC, 1, 0.5), (CD, 1), (MODE, 1), (CONT, 1, 0.5), (CONT, 1, 1.0)])
    assert_rows(got, [[0, big + 1, 3, big + 1, float(big + 1), float(big + 2)]])   # as doubles big and big + 1 are one value


def test_mode_ties_go_to_the_smallest_value():
    rows = [(0, "b"), (0, "a"), (0, "b"), (0, "a"), (0, "c"), (1, 3.0), (1, -0.0), (1, 0.0), (1, 3.0), (1, 0.0), (1, -0.0)]
    assert [r[1] for r in grouped(rows, [0], [(MODE, 1)])] == ["a", -0.0]
    assert same(grouped(rows[5:], [0], [(MODE, 1)])[0][1], -0.0)


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_of_the_operator():
    for group_by, fns in (([], []), ([0] * 8, []), ([0], [(CD, 0)] * 17), ([0], [(9, 0)]), ([0], [(-1, 0)]), ([0], [(DISC, 0, 1.5)]),
                          ([0], [(CONT, 0, -0.1)]), ([0], [(CONT, 0, NAN)]), ([0], [(CD,)]), ([-1], []), ([0], [(CD, -2)])):
        with pytest.raises(ValueError):
            OrderedAggregateOperator(Rows([]), group_by, fns)
    for rows in ([("a", "b")], [("a", True)]):
        with pytest.raises(ValueError):
            grouped(rows, [0], [(CONT, 1, 0.5)])
    OrderedAggregateOperator(Rows([]), [0], [(MODE, 0, 7.0)])      # the fraction is read by the percentiles only


def test_entries_of_the_python_layer():
    assert E.MEDIAN(3) == (N.OSA_PERCENTILE_CONT, 3, 0.5)
    assert E.ordered_agg((N.OSA_MODE, 2)) == (N.OSA_MODE, 2, 0.0) and E.ordered_agg([N.OSA_PERCENTILE_DISC, 1, 1]) == (2, 1, 1.0)
    with pytest.raises(ValueError):
        E.ordered_agg((1,))
    assert (N.OSA_COUNT_DISTINCT, N.OSA_PERCENTILE_CONT, N.OSA_PERCENTILE_DISC, N.OSA_MODE) == (0, 1, 2, 3)
    assert C.sizeof(N.OrderedAgg) == 16


def test_null_pointers_and_the_stats_of_a_fresh_context(native_lib):
    ctx = C.c_void_p()
    assert native_lib.qe_ctx_create(N.DEVICE_NONE, None, C.byref(ctx)) == N.OK
    try:
        fake = C.c_void_p(0x1000)       # never dereferenced: the null checks come first
        fns = (N.OrderedAgg * 1)(N.OrderedAgg(CD, 0, 0.0))
        cols = (C.c_int32 * 1)(0)
        for args in ((ctx, fake, cols, 1, None, 1), (ctx, None, cols, 1, fns, 1), (None, fake, cols, 1, fns, 1), (ctx, fake, None, 1, fns, 1)):
            out = C.c_void_p(0xdead)
            assert native_lib.qe_result_group_ordered(*args, C.byref(out)) == 1
            assert out.value is None                                                  # *out = NULL
        assert native_lib.qe_result_group_ordered(ctx, fake, cols, 1, fns, 1, None) == 1
        stats = (C.c_int64 * 4)()
        assert native_lib.qe_ctx_last_ordered_stats(ctx, None) == 1 and native_lib.qe_ctx_last_ordered_stats(None, stats) == 1
        assert native_lib.qe_ctx_last_ordered_stats(ctx, stats) == N.OK and list(stats) == [0, 0, 0, 0]
    finally:
        native_lib.qe_ctx_destroy(ctx)
