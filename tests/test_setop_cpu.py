"""Set operations without a GPU: the host branch of ``SetOperator`` against answers written out here, the numpy reference of
the device tests (tests/setop_reference.py) against that host branch row for row, and the argument checks of the Python layer
and of qe_result_set_op that need no device."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from queryengine_amd import Column, DataType
from queryengine_amd import native as N
from queryengine_amd.operators import Operator, SetOperator, map as op_map

from setop_reference import merged_dictionary, setop_reference

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
U, I, X = N.SET_UNION, N.SET_INTERSECT, N.SET_EXCEPT
FORMS = [(op, all_) for op in (U, I, X) for all_ in (False, True)]
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Rows(Operator):
    def __init__(self, rows):
        self.rows, self.i, self.opens = [list(r) for r in rows], None, 0

    def open(self):
        self.i = 0
        self.opens += 1

    def close(self):
        self.i = None

    def next(self):
        if self.i >= len(self.rows):
            return None
        self.i += 1
        return self.rows[self.i - 1]


def set_op(left, right, op, all_=False):
    return op_map(SetOperator(Rows(left), Rows(right), op, all_), lambda r: list(r))


def bits(x):
    return struct.pack("<d", x)


def same(a, b):
    """NaN compares by "both NaN"; every other value by bits (so -0.0 is not 0.0, and an int is not a float)."""
    if isinstance(a, float) and isinstance(b, float) and a != a and b != b:
        return True
    if isinstance(a, float) and isinstance(b, float):
        return bits(a) == bits(b)
    return type(a) is type(b) and a == b


def assert_rows(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want), got, want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) and all(same(x, y) for x, y in zip(g, w)), f"{what} row {i}: got {g}, want {w}"


# ---- answers written out ---------------------------------------------------------------------------------------------------------
def test_null_equals_null():
    left = [(None, 1), (None, 1), (2, None)]
    right = [(None, 1), (2, None), (3, 3)]
    assert_rows(set_op(left, right, U), [[None, 1], [2, None], [3, 3]])
    assert_rows(set_op(left, right, U, True), [list(r) for r in left + right])
    assert_rows(set_op(left, right, I), [[None, 1], [2, None]])
    assert_rows(set_op(left, right, I, True), [[None, 1], [2, None]])          # min(2, 1), min(1, 1)
    assert_rows(set_op(left, right, X), [])
    assert_rows(set_op(left, right, X, True), [[None, 1]])                       # 2 - 1
    assert_rows(set_op(right, left, X), [[3, 3]])


def test_every_nan_is_one_value_and_the_first_row_of_the_sequence_comes_out():
    nan1, nan2 = struct.unpack("<2d", struct.pack("<2Q", 0x7ff8000000000001, 0x7ff8000000000002))
    assert bits(nan1) != bits(nan2)
    left, right = [(nan1,), (1.0,)], [(nan2,), (nan2,)]
    for op, all_, count, payload in ((U, False, 2, nan1), (I, False, 1, nan1), (I, True, 1, nan1), (X, False, 1, None), (X, True, 1, None)):
        got = set_op(left, right, op, all_)
        assert len(got) == count, (op, all_, got)
        if payload is not None:
            assert bits(got[-1][0]) == bits(payload), (op, all_)                # NaN sorts last; the left row is the one kept
        else:
            assert got == [[1.0]]
    assert bits(set_op(right, left, U)[-1][0]) == bits(nan2)                     # the other side first: its payload
    got = set_op(right, left, X, True)                                           # 2 - 1 copies, the FIRST of the left's rows
    assert len(got) == 1 and bits(got[0][0]) == bits(nan2)
    got = set_op(left, right, U, True)
    assert [bits(r[0]) for r in got] == [bits(v) for v in (nan1, 1.0, nan2, nan2)]


def test_negative_zero_is_not_zero():
    left, right = [(0.0,), (-0.0,)], [(0.0,)]
    assert_rows(set_op(left, right, U), [[-0.0], [0.0]])                         # Double.compareTo: -0.0 first
    assert_rows(set_op(left, right, I), [[0.0]])
    assert_rows(set_op(left, right, X), [[-0.0]])
    assert_rows(set_op(right, left, X), [])


def test_multiset_counts_below_equal_and_above():
    left = [("z",), ("x",), ("y",), ("z",), ("y",), ("z",)]                      # x 1, y 2, z 3
    right = [("x",), ("y",), ("x",), ("z",), ("x",), ("y",)]                     # x 3, y 2, z 1
    assert_rows(set_op(left, right, I, True), [["x"], ["y"], ["y"], ["z"]])     # min(1, 3), min(2, 2), min(3, 1)
    assert_rows(set_op(left, right, X, True), [["z"], ["z"]])                    # 0, 0, 3 - 1
    assert_rows(set_op(right, left, X, True), [["x"], ["x"]])
    assert_rows(set_op(left, right, U), [["x"], ["y"], ["z"]])
    assert_rows(set_op(left, right, I), [["x"], ["y"], ["z"]])
    assert_rows(set_op(left, right, X), [])
    assert_rows(set_op(left, right, U, True), [list(r) for r in left + right])


def test_empty_sides():
    rows = [(2, True), (1, False), (2, True)]
    distinct = [[1, False], [2, True]]
    ordered = [[1, False], [2, True], [2, True]]
    for op, all_ in FORMS:
        assert set_op([], [], op, all_) == []
    assert_rows(set_op(rows, [], U), distinct)
    assert_rows(set_op([], rows, U), distinct)
    assert_rows(set_op(rows, [], U, True), [list(r) for r in rows])
    assert_rows(set_op([], rows, U, True), [list(r) for r in rows])
    assert set_op(rows, [], I) == [] and set_op([], rows, I) == [] and set_op(rows, [], I, True) == [] and set_op([], rows, I, True) == []
    assert_rows(set_op(rows, [], X), distinct)
    assert_rows(set_op(rows, [], X, True), ordered)
    assert set_op([], rows, X) == [] and set_op([], rows, X, True) == []


def test_left_is_right():
    src = Rows([(2,), (None,), (2,), (1,)])
    distinct = [[None], [1], [2]]

    def run(op, all_):
        return op_map(SetOperator(src, src, op, all_), lambda r: list(r))
    assert_rows(run(U, False), distinct)
    assert_rows(run(I, False), distinct)
    assert_rows(run(I, True), [[None], [1], [2], [2]])                           # min(c, c) = c
    assert run(X, False) == [] and run(X, True) == []
    assert_rows(run(U, True), [[2], [None], [2], [1]] * 2)
    assert src.opens == 6                                                        # drained once per run


# ---- a string under different codes: the merged dictionary ---------------------------------------------------------------------
def test_a_string_under_different_codes_in_the_two_dictionaries():
    entries, table = merged_dictionary(["a", "b"], ["b", "c", "a"])
    assert entries == ["a", "b", "c"] and table.tolist() == [1, 2, 0]
    entries, table = merged_dictionary(["a", "b", "a"], ["a", "c", "c", "b"])   # twice-listed: the left's first code; both of the right's stay
    assert entries == ["a", "b", "a", "c", "c"] and table.tolist() == [0, 3, 4, 1]
    left = [Column(S, np.array([0, 1, 1], dtype=np.int32), None, ["a", "b"])]                     # a b b
    right = [Column(S, np.array([0, 2, 1, 0], dtype=np.int32), None, ["b", "c", "a"])]           # b a c b
    want, stats = setop_reference(left, right, [False], [False], I, True)
    assert want[0].dictionary == ["a", "b", "c"] and want[0].data.tolist() == [0, 1, 1] and stats["translated_columns"] == 1
    want, _ = setop_reference(left, right, [False], [False], X, True)
    assert want[0].data.tolist() == []
    want, _ = setop_reference(right, left, [False], [False], X, True)                              # merged the other way round: b c a
    assert want[0].dictionary == ["b", "c", "a"] and want[0].data.tolist() == [1]
    want, stats = setop_reference(left, right, [False], [False], U, True)
    assert want[0].data.tolist() == [0, 1, 1, 1, 0, 2, 1] and stats["tuples"] == 0
    lrows, rrows = [[c.value(i) for c in left] for i in range(3)], [[c.value(i) for c in right] for i in range(4)]
    assert_rows(set_op(lrows, rrows, I, True), [["a"], ["b"], ["b"]])
    shared, stats = setop_reference(left, left, [False], [False], I)
    assert shared[0].dictionary == ["a", "b"] and stats["translated_columns"] == 0


# ---- the numpy reference equals the host branch ---------------------------------------------------------------------------------
POOLS = {D: [NAN, -0.0, 0.0, INF, 1.5, -2.25], I64: [2 ** 53, 2 ** 53 + 1, -(2 ** 63), 0, 7], I32: [0, -1, 2 ** 31 - 1, 5], B: [False, True]}
NPTYPE = {D: np.float64, I64: np.int64, I32: np.int32, B: bool}
WORDS = ["b", "a", "", "B", "～", "\U0001F600", "aa", "Zü"]
DICT_MODES = ["shared", "reordered", "overlapping", "disjoint", "twice"]


def dictionaries(rng, mode):
    k = int(rng.integers(2, 5))
    left = [WORDS[i] for i in rng.permutation(len(WORDS))[:k]]
    if mode == "shared":
        return left, list(left)
    if mode == "reordered":
        return left, left[::-1]
    if mode == "overlapping":
        return left, left[1:] + [w for w in WORDS if w not in left][:2]
    if mode == "disjoint":
        return left, [w for w in WORDS if w not in left][:3]
    return left + [left[0]], [left[1], "new", left[1], "new"]                      # each side lists a string twice


def side_column(t, rng, values, nullable, dictionary):
    """One side's column from boxed values: without a bitmap a None becomes a value; a string goes to one of its codes in this
    side's dictionary, or (the dictionary does not hold it) to any code."""
    pool = list(range(len(dictionary))) if t == S else POOLS[t]
    valid = np.array([v is not None for v in values], dtype=bool) if nullable else None
    data = []
    for v in values:
        if t == S:
            codes = [i for i, s in enumerate(dictionary) if s == v]
            data.append(codes[int(rng.integers(0, len(codes)))] if codes else pool[int(rng.integers(0, len(pool)))])
        else:
            data.append(pool[int(rng.integers(0, len(pool)))] if v is None else v)
    return Column(t, np.array(data, dtype=np.int32 if t == S else NPTYPE[t]), valid, dictionary if t == S else None)


def random_case(seed):
    """Both sides draw their rows from one small pool of tuples, so that tuples meet across the sides with every cL and cR."""
    rng = np.random.default_rng(seed)
    ncols = int(rng.integers(1, 9))
    types = [[D, I64, I32, B, S][i] for i in rng.integers(0, 5, ncols)]
    types[int(rng.integers(0, ncols))] = [D, I64, I32, B, S][seed % 5]
    dicts = [dictionaries(rng, DICT_MODES[int(rng.integers(0, len(DICT_MODES)))]) if t == S else (None, None) for t in types]
    tuples = []
    for _ in range(int(rng.integers(1, 10))):
        row = []
        for t, (ld, rd) in zip(types, dicts):
            pool = ld + rd if t == S else POOLS[t]
            row.append(None if rng.random() < 0.25 else pool[int(rng.integers(0, len(pool)))])
        tuples.append(row)
    sides = []
    for which in (0, 1):
        picks = rng.integers(0, len(tuples), int(rng.integers(0, 61)))
        sides.append([side_column(t, rng, [tuples[i][c] for i in picks], rng.random() < 0.5, dicts[c][which])
                      for c, t in enumerate(types)])
    return sides[0], sides[1]


def boxed(cols, n):
    return [[c.value(i) for c in cols] for i in range(n)]


@pytest.mark.parametrize("block", range(8))
def test_the_numpy_reference_equals_the_host_branch(block):
    """240 seeded inputs of at most 60 rows a side: all five types, 1 to 8 columns, each side nullable or not, every dictionary
    mode; all six forms each."""
    seen_types, seen_modes = set(), 0
    for seed in range(block * 30, block * 30 + 30):
        left, right = random_case(seed)
        seen_types |= {c.type for c in left}
        lrows, rrows = boxed(left, len(left[0])), boxed(right, len(right[0]))
        for op, all_ in FORMS:
            want, stats = setop_reference(left, right, [c.valid is not None for c in left], [c.valid is not None for c in right], op, all_)
            rows = boxed([Column(w.type, w.data, w.valid, w.dictionary) for w in want], len(want[0].data))
            assert_rows(set_op(lrows, rrows, op, all_), rows, f"seed {seed} op {op} all {all_}")
            assert [w.nullable for w in want] == [l.valid is not None or r.valid is not None for l, r in zip(left, right)]
            seen_modes += stats["translated_columns"]
    assert seen_types == {D, I64, I32, B, S} and seen_modes > 0


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_of_the_operator():
    for op, all_ in ((3, False), (-1, False), (None, False), (1.0, False), (U, 2), (U, -1), (U, None)):
        with pytest.raises(ValueError):
            SetOperator(Rows([]), Rows([]), op, all_)
    for left, right in ((None, Rows([])), (Rows([]), None)):
        with pytest.raises(ValueError):
            SetOperator(left, right, U)
    with pytest.raises(ValueError):
        set_op([(1, 2)], [(1,)], I)                                                # different column counts
    with pytest.raises(ValueError):
        set_op([(1,)], [("a",)], I)                                                # a column whose types differ
    with pytest.raises(ValueError):
        set_op([()], [()], I)                                                      # zero columns
    SetOperator(Rows([]), Rows([]), X, 1)


def test_constants_of_the_python_layer():
    assert (N.SET_UNION, N.SET_INTERSECT, N.SET_EXCEPT) == (0, 1, 2)
    text = open(os.path.join(ROOT, "queryengine_amd", "csrc", "qe_kernels.h")).read()
    assert N.SETOP_BLOCKS == int(re.search(r"constexpr\s+int\s+kSetopBlocks\s*=\s*(\d+)\s*;", text).group(1))
    header = open(os.path.join(ROOT, "include", "qe_hip.h")).read()
    assert re.search(r"QE_SET_UNION\s*=\s*0\s*,\s*QE_SET_INTERSECT\s*=\s*1\s*,\s*QE_SET_EXCEPT\s*=\s*2", header)


def test_null_pointers_and_the_stats_of_a_fresh_context(native_lib):
    ctx = C.c_void_p()
    assert native_lib.qe_ctx_create(N.DEVICE_NONE, None, C.byref(ctx)) == N.OK
    try:
        fake = C.c_void_p(0x1000)       # never dereferenced: the null checks come first
        for args in ((None, fake, fake, 0, 0), (ctx, None, fake, 0, 0), (ctx, fake, None, 0, 0)):
            out = C.c_void_p(0xdead)
            assert native_lib.qe_result_set_op(*args, C.byref(out)) == 1
            assert out.value is None                                                  # *out = NULL
        assert native_lib.qe_result_set_op(ctx, fake, fake, 0, 0, None) == 1
        stats = (C.c_int64 * 4)()
        assert native_lib.qe_ctx_last_set_stats(ctx, None) == 1 and native_lib.qe_ctx_last_set_stats(None, stats) == 1
        assert native_lib.qe_ctx_last_set_stats(ctx, stats) == N.OK and list(stats) == [0, 0, 0, 0]
    finally:
        native_lib.qe_ctx_destroy(ctx)
