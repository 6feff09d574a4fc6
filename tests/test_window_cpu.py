"""The window operator without a GPU: the host branch of ``WindowOperator`` against hand-written expectations, the numpy
reference of the device tests (tests/window_reference.py) against that host branch value for value, and the argument errors
of qe_result_window that need no device."""
import ctypes as C
import math
import struct

import numpy as np
import pytest

from queryengine_amd import Column, DataType
from queryengine_amd import native as N
from queryengine_amd.operators import Operator, WindowOperator, map as op_map

from window_reference import window_reference

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
NAN, INF = float("nan"), float("inf")
STRINGS = ["b", "a", "", "B", "～", "\U0001F600", "aa", "Zü", "zz", "a "]
DOUBLES = np.array([0.0, -0.0, 1.5, -1.5, float("nan"), float("inf"), -float("inf"), 1e300, -1e-300, 3.0])
INT64S = np.array([0, -1, 1, 2 ** 63 - 1, -(2 ** 63), 2 ** 53 + 1, 2 ** 63 - 2], dtype=np.int64)
ALL_FNS = [(N.WIN_ROW_NUMBER,), (N.WIN_RANK,), (N.WIN_DENSE_RANK,), (N.WIN_SUM, 2), (N.WIN_COUNT, 3), (N.WIN_MIN, 2), (N.WIN_MAX, 2),
           (N.WIN_AVG, 2), (N.WIN_LAG, 3, 1), (N.WIN_LEAD, 2, 2)]


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


def window(rows, partition_by, order_by, functions):
    return op_map(WindowOperator(Rows([list(r) for r in rows]), partition_by, order_by, functions), lambda r: list(r))


def bits(v):
    return struct.pack("<d", v) if isinstance(v, float) else v


def same(a, b):
    """NaN compares by "both NaN"; every other value by bits (so -0.0 is not 0.0, and an int is not a float)."""
    if isinstance(a, float) and isinstance(b, float) and a != a and b != b:
        return True
    return type(a) is type(b) and bits(a) == bits(b)


def assert_rows(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and all(same(x, y) for x, y in zip(g, w)), f"row {i}: got {g}, want {w}"


# (partition key, order key, row id)
RANK_ROWS = [("x", 2.0, 0), ("y", 1.0, 1), ("x", 1.0, 2), (None, 5.0, 3), ("x", 2.0, 4), ("x", None, 5), ("y", 1.0, 6),
             (None, 5.0, 7), ("x", 3.0, 8), ("x", 1.0, 9), ("y", None, 10), ("x", 2.0, 11)]


def test_ranks_with_ties_and_a_null_partition_key():
    got = window(RANK_ROWS, [0], [(1, False)], [(N.WIN_ROW_NUMBER,), (N.WIN_RANK,), (N.WIN_DENSE_RANK,)])
    # NULL is a partition of its own and comes first; inside a partition NULL order keys first, ties in input order
    want = [[None, 5.0, 3, 1, 1, 1], [None, 5.0, 7, 2, 1, 1],
            ["x", None, 5, 1, 1, 1], ["x", 1.0, 2, 2, 2, 2], ["x", 1.0, 9, 3, 2, 2], ["x", 2.0, 0, 4, 4, 3], ["x", 2.0, 4, 5, 4, 3],
            ["x", 2.0, 11, 6, 4, 3], ["x", 3.0, 8, 7, 7, 4],
            ["y", None, 10, 1, 1, 1], ["y", 1.0, 1, 2, 2, 2], ["y", 1.0, 6, 3, 2, 2]]
    assert_rows(got, want)


def test_descending_order_key_puts_null_last():
    got = window(RANK_ROWS, [0], [(1, True)], [(N.WIN_RANK,)])
    assert [r[2] for r in got] == [3, 7, 8, 0, 4, 11, 2, 9, 5, 1, 6, 10]
    assert [r[3] for r in got] == [1, 1, 1, 2, 2, 2, 5, 5, 7, 1, 1, 3]


def test_no_order_keys_keeps_input_order_and_makes_every_row_a_peer():
    got = window(RANK_ROWS, [0], [], [(N.WIN_ROW_NUMBER,), (N.WIN_RANK,), (N.WIN_DENSE_RANK,)])
    assert [r[2] for r in got] == [3, 7, 0, 2, 4, 5, 8, 9, 11, 1, 6, 10]
    assert [r[3:] for r in got] == [[1, 1, 1], [2, 1, 1]] + [[i, 1, 1] for i in range(1, 8)] + [[i, 1, 1] for i in range(1, 4)]


def test_no_keys_at_all_is_one_partition_in_input_order():
    got = window(RANK_ROWS, [], [], [(N.WIN_ROW_NUMBER,), (N.WIN_COUNT, 1)])
    assert [r[2] for r in got] == list(range(12))
    assert [r[3] for r in got] == list(range(1, 13))
    assert [r[4] for r in got] == [1, 2, 3, 4, 5, 5, 6, 7, 8, 9, 9, 10]


def test_lag_and_lead_at_partition_edges_and_offset_zero():
    rows = [("a", 1, "p"), ("a", 2, None), ("a", 3, "q"), ("b", 4, "r"), ("b", 5, "s")]
    got = window(rows, [0], [(1, False)], [(N.WIN_LAG, 2, 1), (N.WIN_LEAD, 2, 1), (N.WIN_LAG, 2, 0), (N.WIN_LEAD, 1, 2), (N.WIN_LAG, 1, 7)])
    want = [["a", 1, "p", None, None, "p", 3, None], ["a", 2, None, "p", "q", None, None, None], ["a", 3, "q", None, None, "q", None, None],
            ["b", 4, "r", None, "s", "r", None, None], ["b", 5, "s", "r", None, "s", None, None]]
    assert_rows(got, want)


def test_running_aggregates_and_their_special_values():
    rows = [(1, None), (1, None), (1, 2.5), (1, None), (1, -0.5),       # NULL before the first valid value, NULLs skipped
            (2, -0.0), (2, -0.0), (2, 0.0),                            # only -0.0 sums to +0.0; MIN -0.0, MAX 0.0
            (3, 1.0), (3, INF), (3, 2.0), (3, -INF), (3, 3.0),         # one infinity stays, both give NaN to the end
            (4, 5.0), (4, NAN), (4, 1.0)]                              # NaN persists in SUM and wins MIN / MAX
    got = window(rows, [0], [], [(N.WIN_SUM, 1), (N.WIN_COUNT, 1), (N.WIN_MIN, 1), (N.WIN_MAX, 1), (N.WIN_AVG, 1)])
    want = [[None, 0, None, None, None], [None, 0, None, None, None], [2.5, 1, 2.5, 2.5, 2.5], [2.5, 1, 2.5, 2.5, 2.5], [2.0, 2, -0.5, 2.5, 1.0],
            [0.0, 1, -0.0, -0.0, 0.0], [0.0, 2, -0.0, -0.0, 0.0], [0.0, 3, -0.0, 0.0, 0.0],
            [1.0, 1, 1.0, 1.0, 1.0], [INF, 2, 1.0, INF, INF], [INF, 3, 1.0, INF, INF], [NAN, 4, -INF, INF, NAN], [NAN, 5, -INF, INF, NAN],
            [5.0, 1, 5.0, 5.0, 5.0], [NAN, 2, NAN, NAN, NAN], [NAN, 3, NAN, NAN, NAN]]
    assert_rows([r[2:] for r in got], want)


def test_count_over_a_string_column_and_integer_arguments():
    rows = [("k", "s", 3), ("k", None, 4), ("k", "t", None), ("k", "s", -9)]
    got = window(rows, [0], [], [(N.WIN_COUNT, 1), (N.WIN_SUM, 2), (N.WIN_MAX, 2)])
    assert_rows([r[3:] for r in got], [[1, 3.0, 3.0], [1, 7.0, 4.0], [2, 7.0, 4.0], [3, -2.0, 4.0]])


def test_double_partition_keys_nan_is_one_value_and_the_zeros_are_two():
    rows = [(NAN, 0), (0.0, 1), (-0.0, 2), (float.fromhex("0x1.8p+1023") * 0 + NAN, 3), (0.0, 4), (-0.0, 5)]
    got = window(rows, [0], [], [(N.WIN_ROW_NUMBER,)])
    assert [r[1] for r in got] == [2, 5, 1, 4, 0, 3]
    assert [r[2] for r in got] == [1, 2, 1, 2, 1, 2]


def test_bad_arguments_of_the_operator():
    with pytest.raises(ValueError):
        WindowOperator(Rows([]), [0], [], [])
    with pytest.raises(ValueError):
        WindowOperator(Rows([]), [0], [], [(99,)])
    with pytest.raises(ValueError):
        WindowOperator(Rows([]), [0], [], [(N.WIN_LAG, 0, -1)])
    with pytest.raises(ValueError):
        window([("a", "b")], [0], [], [(N.WIN_SUM, 1)])


# ---- the numpy reference equals the host branch ---------------------------------------------------------------------------
def make_key(t, rng, n, coarse, null_share=0.1):
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


def reference_rows(cols, partition_by, order_by, functions):
    want, _, _ = window_reference(cols, [c.valid is not None for c in cols], partition_by, order_by, functions)
    out = []
    for j in range(len(cols[0])):
        row = [Column(w.type, w.data, w.valid, w.dictionary).value(j) for w in want]
        for k, f in enumerate(functions):
            if f[0] == N.WIN_COUNT:
                row[len(cols) + k] = int(row[len(cols) + k])
        out.append(row)
    return out


@pytest.mark.parametrize("ptype", [D, I64, I32, B, S], ids=lambda t: t.name)
@pytest.mark.parametrize("otype", [D, S, I64], ids=lambda t: t.name)
def test_the_numpy_reference_equals_the_host_branch(ptype, otype):
    rng = np.random.default_rng(1000 + int(ptype) * 10 + int(otype))
    n = 900
    # (partition key, order key, DOUBLE value with the special pool, a payload of the order key's type, row id)
    cols = [make_key(ptype, rng, n, coarse=True), make_key(otype, rng, n, coarse=True), make_key(D, rng, n, coarse=False),
            make_key(otype, rng, n, coarse=False), Column(I64, np.arange(n, dtype=np.int64))]
    rows = [[c.value(i) for c in cols] for i in range(n)]
    for part, order in (([0], [(1, False)]), ([0], [(1, True)]), ([0, 1], []), ([], [(1, True), (0, False)]), ([], [])):
        assert_rows(window(rows, part, order, ALL_FNS), reference_rows(cols, part, order, ALL_FNS))


def test_the_numpy_reference_on_integer_and_boolean_arguments_and_tiny_inputs():
    rng = np.random.default_rng(5)
    for n in (0, 1, 2, 65):
        cols = [make_key(I32, rng, n, coarse=True), make_key(I64, rng, n, coarse=False), make_key(I32, rng, n, coarse=False),
                make_key(B, rng, n, coarse=True), Column(I64, np.arange(n, dtype=np.int64))]
        fns = [(N.WIN_SUM, 1), (N.WIN_AVG, 2), (N.WIN_MIN, 1), (N.WIN_MAX, 2), (N.WIN_COUNT, 3), (N.WIN_LAG, 3, 2), (N.WIN_LEAD, 3, 0),
               (N.WIN_LEAD, 0, 64), (N.WIN_DENSE_RANK,)]
        rows = [[c.value(i) for c in cols] for i in range(n)]
        assert_rows(window(rows, [0], [(3, True)], fns), reference_rows(cols, [0], [(3, True)], fns))


# ---- argument errors that need no device -------------------------------------------------------------------------------------
def test_null_pointers_are_invalid_arguments(native_lib):
    ctx = C.c_void_p()
    assert native_lib.qe_ctx_create(N.DEVICE_NONE, None, C.byref(ctx)) == N.OK
    try:
        fake = C.c_void_p(0x1000)       # never dereferenced: the null checks come first
        fns = (N.WindowFn * 1)(N.WindowFn(N.WIN_ROW_NUMBER, 0, 0))
        out = C.c_void_p(0xdead)
        assert native_lib.qe_result_window(ctx, fake, None, 0, None, 0, None, 1, C.byref(out)) == 1     # null fns
        assert out.value is None                                                                        # *out = NULL
        assert native_lib.qe_result_window(ctx, fake, None, 0, None, 0, fns, 1, None) == 1              # null out
        out = C.c_void_p(0xdead)
        assert native_lib.qe_result_window(ctx, None, None, 0, None, 0, fns, 1, C.byref(out)) == 1      # null result
        assert out.value is None
        assert native_lib.qe_result_window(None, fake, None, 0, None, 0, fns, 1, C.byref(out)) == 1     # null context
        stats = (C.c_int64 * 4)()
        assert native_lib.qe_ctx_last_window_stats(ctx, None) == 1
        assert native_lib.qe_ctx_last_window_stats(ctx, stats) == N.OK and list(stats) == [0, 0, 0, 0]
    finally:
        native_lib.qe_ctx_destroy(ctx)
