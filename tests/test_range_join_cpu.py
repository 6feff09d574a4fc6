"""The range join without a GPU: the host branch of ``RangeJoinOperator`` against answers written out here, the numpy reference
of the device tests (tests/range_join_reference.py) against that host branch row for row, the argument checks of the Python
layer and of qe_result_range_join that need no device, and the operator's choice between the device and the host.

A planning-only context cannot hold a result, so the ABI is reached here with handles that are never dereferenced: the null
pointers and every error that qe_result_range_join decides from its scalar arguments alone (nby, the strict flags, join_type,
the column counts).  The errors that need a result to look at -- a column out of range, paired by columns of different types,
the types of the value columns -- are in tests/test_gpu_range_join.py.  Not tested anywhere: QE_ERR_HIP on a planning-only
context (it would need a result there), a STRING by column without a dictionary (the ABI cannot build one)."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from queryengine_amd import Column, DataType
from queryengine_amd import native as N
from queryengine_amd.operators import DeviceResultOperator, RangeJoinOperator, map as op_map

from range_join_reference import range_reference
from test_setop_cpu import POOLS, Rows, assert_rows, boxed, dictionaries, side_column, DICT_MODES

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
INNER, LEFT, SEMI, ANTI = N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI
JOINS = [INNER, LEFT, SEMI, ANTI]
STRICTS = [(False, False), (False, True), (True, False), (True, True)]
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1


def rjoin(left, right, left_by, right_by, lo, hi, on, lo_strict=False, hi_strict=False, join_type=INNER, left_out=None, right_out=None):
    return op_map(RangeJoinOperator(Rows(left), Rows(right), left_by, right_by, lo, hi, on, lo_strict, hi_strict, join_type,
                                    left_out, right_out), lambda r: list(r))


# ---- answers written out ---------------------------------------------------------------------------------------------------------
def test_quotes_around_trades():
    quotes = [["a", 1, 10.0], ["b", 2, 20.0], ["a", 3, 11.0], ["a", 7, 12.0], ["b", 9, 21.0], ["a", 3, 13.0]]   # symbol, time, price
    trades = [["a", 5, 0, 5], ["b", 9, 4, 9], ["c", 5, 0, 9], ["a", 3, 3, 8], ["b", 1, 0, 1]]                 # symbol, time, t - 5, t [+ 5]
    assert_rows(rjoin(trades, quotes, [0], [0], 2, 3, 1, left_out=[0, 1], right_out=[1, 2]),
                [["a", 5, 1, 10.0], ["a", 5, 3, 11.0], ["a", 5, 3, 13.0], ["b", 9, 9, 21.0], ["a", 3, 3, 11.0], ["a", 3, 3, 13.0], ["a", 3, 7, 12.0]])
    assert_rows(rjoin(trades, quotes, [0], [0], 2, 3, 1, join_type=LEFT, left_out=[0, 1], right_out=[2]),
                [["a", 5, 10.0], ["a", 5, 11.0], ["a", 5, 13.0], ["b", 9, 21.0], ["c", 5, None], ["a", 3, 11.0], ["a", 3, 13.0], ["a", 3, 12.0],
                 ["b", 1, None]])
    assert_rows(rjoin(trades, quotes, [0], [0], 2, 3, 1, join_type=SEMI, left_out=[0, 1]), [["a", 5], ["b", 9], ["a", 3]])
    assert_rows(rjoin(trades, quotes, [0], [0], 2, 3, 1, join_type=ANTI, left_out=[0, 1]), [["c", 5], ["b", 1]])
    assert_rows(rjoin(trades[:1], quotes, [], [], 2, 3, 1, left_out=[1], right_out=[0, 1]),          # no by column: one partition
                [[5, "a", 1], [5, "b", 2], [5, "a", 3], [5, "a", 3]])
    assert rjoin(trades, quotes, [0], [0], 2, 3, 1, join_type=SEMI) == [t for t in trades if t[0] != "c" and t[1] != 1]   # every left column


def test_the_four_strict_combinations_on_equal_values():
    right = [[3, 0], [5, 1], [5, 2], [7, 3], [9, 4], [7, 5]]                                          # on, row id
    left = [[5, 7]]
    ids = lambda ls, hs: [r[2] for r in rjoin(left, right, [], [], 0, 1, 0, ls, hs, right_out=[1])]   # noqa: E731
    assert ids(False, False) == [1, 2, 3, 5] and ids(True, False) == [3, 5] and ids(False, True) == [1, 2] and ids(True, True) == []
    left = [[3, 9]]
    assert ids(False, False) == [0, 1, 2, 3, 5, 4] and ids(True, True) == [1, 2, 3, 5]


def test_an_empty_interval_a_reversed_one_and_lo_equal_to_hi():
    right = [[4, 0], [5, 1], [5, 2], [6, 3]]
    for ls, hs in STRICTS:
        assert rjoin([[6, 4]], right, [], [], 0, 1, 0, ls, hs) == []                                  # reversed
        assert rjoin([[6, 4]], right, [], [], 0, 1, 0, ls, hs, LEFT, right_out=[1]) == [[6, 4, None]]
        assert rjoin([[6, 4]], right, [], [], 0, 1, 0, ls, hs, ANTI) == [[6, 4]]
        got = rjoin([[5, 5]], right, [], [], 0, 1, 0, ls, hs, right_out=[1])                          # lo == hi: equality unless an end is strict
        assert got == ([[5, 5, 1], [5, 5, 2]] if (ls, hs) == (False, False) else [])
        got = rjoin([[5]], right, [], [], 0, 0, 0, ls, hs, right_out=[1])                             # the same column as both bounds
        assert got == ([[5, 1], [5, 2]] if (ls, hs) == (False, False) else [])
    assert rjoin([[4, 5]], right, [], [], 0, 1, 0, True, True) == []                                  # nothing strictly between


def test_special_values_as_bounds_and_as_on():
    ons = [NAN, -0.0, 0.0, INF, -INF, 1.5, NAN]
    right = [[v, i] for i, v in enumerate(ons)]
    ids = lambda lo, hi, ls=False, hs=False: [r[2] for r in rjoin([[lo, hi]], right, [], [], 0, 1, 0, ls, hs, right_out=[1])]   # noqa: E731
    assert ids(-INF, INF) == [4, 1, 2, 5, 3] and ids(-INF, NAN) == [4, 1, 2, 5, 3, 0, 6]              # NaN greatest, all NaNs equal
    assert ids(NAN, NAN) == [0, 6] and ids(NAN, NAN, True) == [] and ids(INF, NAN, True, False) == [0, 6]
    assert ids(-0.0, 0.0) == [1, 2] and ids(-0.0, 0.0, True) == [2] and ids(-0.0, 0.0, False, True) == [1]   # -0.0 < 0.0
    assert ids(0.0, -0.0) == [] and ids(0.0, 0.0) == [2] and ids(-0.0, -0.0) == [1]
    assert ids(-INF, -INF) == [4] and ids(-INF, INF, True, True) == [1, 2, 5] and ids(NAN, INF) == []
    big = 2 ** 53
    assert float(big) == float(big + 1)                                                               # equal as doubles, apart as INT64
    right = [[big + 1, 0], [big, 1], [-(2 ** 63), 2], [2 ** 63 - 1, 3]]
    assert ids(big, big) == [1] and ids(big + 1, big + 1) == [0] and ids(big, big + 1, True) == [0] and ids(big, big + 1, False, True) == [1]
    assert ids(-(2 ** 63), 2 ** 63 - 1) == [2, 1, 0, 3] and ids(-(2 ** 63), 2 ** 63 - 1, True, True) == [1, 0]


def test_a_null_matches_nothing_and_hides_nothing():
    right = [["k", 1, 0], ["k", None, 1], [None, 2, 2], ["k", 3, 3]]                                  # by, on, row id
    assert rjoin([["k", 0, 9]], right, [0], [0], 1, 2, 1, right_out=[2]) == [["k", 0, 9, 0], ["k", 0, 9, 3]]   # not the NULL on, and past it
    for row in (["k", None, 9], ["k", 0, None], [None, 0, 9], ["k", None, None]):
        assert rjoin([row], right, [0], [0], 1, 2, 1) == [] and rjoin([row], right, [0], [0], 1, 2, 1, join_type=SEMI) == []
        assert rjoin([row], right, [0], [0], 1, 2, 1, join_type=ANTI) == [row]                        # a NULL key counts as no match
        assert rjoin([row], right, [0], [0], 1, 2, 1, join_type=LEFT, right_out=[2]) == [row + [None]]
    assert rjoin([[None, 0, 9]], right, [], [], 1, 2, 1, right_out=[2]) == [[None, 0, 9, 0], [None, 0, 9, 2], [None, 0, 9, 3]]   # not a by column


def test_by_keys_compare_like_join_keys_and_never_leak():
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000002))[0]
    right = [[NAN, 1, 0], [0.0, 1, 1], [-0.0, 5, 2], [NAN, 2, 3], [1.0, 1, 4]]
    left = [[nan2, 0, 9], [-0.0, 0, 9], [0.0, 0, 9], [1.5, 0, 9]]
    got = rjoin(left, right, [0], [0], 1, 2, 1, join_type=LEFT, left_out=[], right_out=[2])
    assert got == [[0], [3], [2], [1], [None]]
    # partitions next to each other in the sort, every interval wide open: nothing of a neighbour comes along
    right = [[p, v, 10 * p + v] for p in (1, 2, 3) for v in (0, 1, 2)]
    left = [[2, -100, 100], [4, -100, 100], [0, -100, 100]]
    assert rjoin(left, right, [0], [0], 1, 2, 1, right_out=[2]) == [[2, -100, 100, 20], [2, -100, 100, 21], [2, -100, 100, 22]]
    same = [[1, 10, 30], [2, 20, 20], [1, 30, 10]]                                                   # a source against itself
    src = Rows(same)
    got = op_map(RangeJoinOperator(src, src, [0], [0], 1, 2, 1, False, False, LEFT, [1], [1]), list)
    assert got == [[10, 10], [10, 30], [20, 20], [30, None]] and src.opens == 1


# ---- the numpy reference equals the host branch ---------------------------------------------------------------------------------
VALUE_POOLS = {D: [NAN, -0.0, 0.0, INF, -INF, 1.5, -2.25, 7.0], I64: [2 ** 53, 2 ** 53 + 1, -(2 ** 63), 2 ** 63 - 1, 0, 7, -3],
               I32: [0, -1, 2 ** 31 - 1, -(2 ** 31), 5, 6]}
TAGS = ["t0", "", "täg"]
OUTS = [[0], [0, 1], [1, 0, 0], [], [2, 0]]         # of (row id, tag, value)


def random_case(seed):
    """Both sides draw their by tuples from one small pool and their values from a pool of special values, so that partitions
    and equal values meet across the sides.  Left columns: by.., lo, hi, row id, tag; right columns: row id, tag, on, by.."""
    rng = np.random.default_rng(seed)
    nby = [0, 1, 1, 2, 3, 7][int(rng.integers(0, 6))]
    types = [[D, I64, I32, B, S][i] for i in rng.integers(0, 5, nby)]
    if nby:
        types[int(rng.integers(0, nby))] = [D, I64, I32, B, S][seed % 5]
    value_type = [D, I64, I32][(seed // 5) % 3]
    dicts = [dictionaries(rng, DICT_MODES[int(rng.integers(0, len(DICT_MODES)))]) if t == S else (None, None) for t in types]
    tuples = []
    for _ in range(int(rng.integers(1, 5))):
        row = []
        for t, (ld, rd) in zip(types, dicts):
            pool = ld + rd if t == S else POOLS[t]
            row.append(None if rng.random() < 0.12 else pool[int(rng.integers(0, len(pool)))])
        tuples.append(row)
    pool = VALUE_POOLS[value_type]

    def values(n, null_share):
        return side_column(value_type, rng, [None if rng.random() < null_share else pool[int(rng.integers(0, len(pool)))] for _ in range(n)],
                           rng.random() < 0.6, None)
    sides = []
    for which in (0, 1):
        n = int(rng.integers(0, 41))
        picks = rng.integers(0, len(tuples), n)
        by = [side_column(t, rng, [tuples[i][c] for i in picks], rng.random() < 0.5, dicts[c][which]) for c, t in enumerate(types)]
        rowid = Column(I64, np.arange(n, dtype=np.int64))
        tag = Column(S, rng.integers(0, len(TAGS), n).astype(np.int32), (rng.random(n) > 0.3) if n else None, TAGS)
        sides.append(by + [values(n, 0.1), values(n, 0.1), rowid, tag] if which == 0 else [rowid, tag, values(n, 0.15)] + by)
    same_bound = seed % 7 == 3                       # lo and hi the same column
    left_out = [[nby + 2, nby + 3, nby][c] for c in OUTS[int(rng.integers(0, len(OUTS)))]]
    right_out = [[0, 1, 2][c] for c in OUTS[int(rng.integers(0, len(OUTS)))]]
    if not left_out:
        left_out = [nby + 2]                          # SEMI and ANTI have only left columns
    return dict(left=sides[0], right=sides[1], left_by=list(range(nby)), right_by=list(range(3, 3 + nby)), lo=nby, hi=nby if same_bound else nby + 1,
                on=2, left_out=left_out, right_out=right_out, value_type=value_type, types=types)


@pytest.mark.parametrize("block", range(12))
def test_the_numpy_reference_equals_the_host_branch(block):
    """300 seeded inputs of at most 40 rows a side, all four join types under all four strict combinations each: every value
    type, all five by types, 0 to 7 by columns, each column nullable or not, every dictionary mode, NaN / +-0.0 / +-Inf and
    INT64 values that differ only beyond 2^53, lo and hi as one column."""
    seen_by, seen_value, pairs, unmatched = set(), set(), 0, 0
    for seed in range(block * 25, block * 25 + 25):
        q = random_case(seed)
        left, right = q["left"], q["right"]
        seen_by |= set(q["types"])
        seen_value.add(q["value_type"])
        lrows, rrows = boxed(left, len(left[0])), boxed(right, len(right[0]))
        for join_type in JOINS:
            right_out = q["right_out"] if join_type in (INNER, LEFT) else []
            for lo_strict, hi_strict in STRICTS:
                want, stats = range_reference(left, right, [c.valid is not None for c in left], [c.valid is not None for c in right], q["left_by"],
                                              q["right_by"], q["lo"], q["hi"], q["on"], lo_strict, hi_strict, join_type, q["left_out"], right_out)
                rows = boxed([Column(w.type, w.data, w.valid, w.dictionary) for w in want], len(want[0].data))
                got = rjoin(lrows, rrows, q["left_by"], q["right_by"], q["lo"], q["hi"], q["on"], lo_strict, hi_strict, join_type,
                            q["left_out"], right_out)
                assert_rows(got, rows, f"seed {seed} join {join_type} strict {lo_strict} {hi_strict}")
                assert len(got) == stats["output_rows"] and (stats["left_rows"], stats["right_rows"]) == (len(lrows), len(rrows))
                assert [w.nullable for w in want] == [left[c].valid is not None for c in q["left_out"]] + \
                    [right[c].valid is not None or join_type == LEFT for c in right_out]
                for w in want[len(q["left_out"]):]:
                    assert w.zero_at is not None and not (w.valid & w.zero_at).any() and not w.data[w.zero_at].any()
                if join_type == LEFT:                   # the row ids of the INNER form: how often each left row comes out
                    ids = rjoin(lrows, rrows, q["left_by"], q["right_by"], q["lo"], q["hi"], q["on"], lo_strict, hi_strict, INNER, [len(q["types"]) + 2], [])
                    assert stats["longest"] == max(np.bincount(np.array([r[0] for r in ids], dtype=np.int64), minlength=1))
                    pairs += len(ids)
                    unmatched += len(got) - len(ids)
    assert seen_by == {D, I64, I32, B, S} and seen_value == {D, I64, I32} and pairs > 100 and unmatched > 100


def test_the_stats_of_the_reference():
    left = [Column(I32, np.array([1, 5, 9], dtype=np.int32)), Column(I32, np.array([4, 5, 0], dtype=np.int32))]
    right = [Column(I32, np.array([2, 3, 5, 5, 1], dtype=np.int32))]
    want, stats = range_reference(left, right, [False, False], [False], [], [], 0, 1, 0, False, False, INNER, [0], [0])
    assert stats == {"left_rows": 3, "right_rows": 5, "output_rows": 5, "longest": 3} and want[1].data.tolist() == [1, 2, 3, 5, 5]
    _, stats = range_reference(left, right, [False, False], [False], [], [], 0, 1, 0, False, False, LEFT, [0], [0])
    assert stats["output_rows"] == 6
    _, stats = range_reference(left, right, [False, False], [False], [], [], 0, 1, 0, False, False, ANTI, [0], [])
    assert stats == {"left_rows": 3, "right_rows": 5, "output_rows": 1, "longest": 3}
    none = [Column(I32, np.zeros(0, dtype=np.int32))]
    want, stats = range_reference(none, none, [False], [False], [], [], 0, 0, 0, True, True, LEFT, [0], [0])
    assert stats == {"left_rows": 0, "right_rows": 0, "output_rows": 0, "longest": 0} and [w.nullable for w in want] == [False, True]


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_of_the_operator():
    ok = dict(left_by=[0], right_by=[0], left_lo=1, left_hi=2, right_on=1)
    for bad in (dict(lo_strict=2), dict(lo_strict=None), dict(hi_strict=2), dict(hi_strict=None), dict(join_type=4), dict(join_type=-1),
                dict(join_type=None), dict(join_type=True), dict(left_by=[0, 1]), dict(left_by=list(range(8)), right_by=list(range(8))),
                dict(left_out=[], right_out=[]), dict(join_type=SEMI, right_out=[0]), dict(join_type=ANTI, right_out=[0]),
                dict(join_type=SEMI, left_out=[]), dict(join_type=ANTI, left_out=[], right_out=[])):
        with pytest.raises(ValueError):
            RangeJoinOperator(Rows([]), Rows([]), **{**ok, **bad})
    for left, right in ((None, Rows([])), (Rows([]), None)):
        with pytest.raises(ValueError):
            RangeJoinOperator(left, right, **ok)
    RangeJoinOperator(Rows([]), Rows([]), **{**ok, **dict(join_type=SEMI, right_out=[])})
    with pytest.raises(ValueError):
        rjoin([[1, "x", "y"]], [[1, "y"]], [0], [0], 1, 2, 1)                      # value columns that are not numeric
    with pytest.raises(ValueError):
        rjoin([[1, True, True]], [[1, True]], [0], [0], 1, 2, 1)
    with pytest.raises(ValueError):
        rjoin([[1, 2, 3]], [[1, 2.0]], [0], [0], 1, 2, 1)                          # whose type differs between the sides
    with pytest.raises(ValueError):
        rjoin([[1, 2, 3.0]], [[1, 2]], [0], [0], 1, 2, 1)                          # or between the bounds
    with pytest.raises(ValueError):
        rjoin([[1, 2, 3]], [], [0], [0], 1, 2, 1, join_type=LEFT)                  # LEFT, no right row, right_out not given
    assert rjoin([[1, 2, 3]], [], [0], [0], 1, 2, 1, join_type=LEFT, right_out=[0, 1]) == [[1, 2, 3, None, None]]
    assert rjoin([[1, 2, 3]], [], [0], [0], 1, 2, 1) == [] and rjoin([], [[1, 2]], [0], [0], 1, 2, 1, join_type=LEFT) == []
    assert rjoin([[1, 2, 3]], [], [0], [0], 1, 2, 1, join_type=ANTI) == [[1, 2, 3]]


def test_constants_of_the_python_layer():
    assert (N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI) == (0, 1, 2, 3)
    text = open(os.path.join(ROOT, "queryengine_amd", "csrc", "qe_kernels.h")).read()
    assert N.RANGE_BLOCKS == int(re.search(r"constexpr\s+int\s+kRangeBlocks\s*=\s*(\d+)\s*;", text).group(1))
    assert N.RANGE_EXPAND_TILE == int(re.search(r"constexpr\s+int\s+kRangeExpandTile\s*=\s*(\d+)\s*;", text).group(1))
    kernels = open(os.path.join(ROOT, "queryengine_amd", "csrc", "qe_range.hip")).read()
    assert "dim3(256)" in kernels and "dim3(128)" not in kernels and "dim3(512)" not in kernels     # RANGE_BLOCKS counts blocks of 256 lanes
    csrc = os.path.join(ROOT, "queryengine_amd", "csrc")
    callers = sorted(f for f in os.listdir(csrc) if f.endswith(".cpp") and "launch_asof_eligible(" in open(os.path.join(csrc, f)).read())
    assert callers == ["qe_two_sided.cpp"] and "void asof_eligible" not in kernels                  # the eligibility kernel is reused, not copied
    header = open(os.path.join(ROOT, "include", "qe_hip.h")).read()
    assert re.search(r"QE_JOIN_INNER\s*=\s*0\s*,\s*QE_JOIN_LEFT\s*=\s*1\s*,\s*QE_JOIN_SEMI\s*=\s*2\s*,\s*QE_JOIN_ANTI\s*=\s*3", header)


@pytest.fixture()
def plan_ctx(native_lib):
    """A planning-only context: no device, so no result can live on it."""
    ctx = C.c_void_p()
    assert native_lib.qe_ctx_create(N.DEVICE_NONE, None, C.byref(ctx)) == N.OK
    yield ctx
    native_lib.qe_ctx_destroy(ctx)


def call_range(lib, ctx, left, right, nby=1, lo_strict=0, hi_strict=0, join_type=INNER, nleft_out=1, nright_out=1, by=True, outs=True, out=True):
    cols = (C.c_int32 * 8)(*range(8))
    res = C.c_void_p(0xdead)
    st = lib.qe_result_range_join(ctx, left, right, cols if by else None, cols if by else None, nby, 0, 0, 0, lo_strict, hi_strict, join_type,
                                  cols if outs else None, nleft_out, cols if outs else None, nright_out, C.byref(res) if out else None)
    if out:
        assert res.value is None, "*out must be NULL after an error"
    return st


def test_errors_that_need_no_result(native_lib, plan_ctx):
    lib = native_lib
    fake = C.c_void_p(0x1000)           # never dereferenced: every check below comes before the first look at a result
    for args in ((None, fake, fake), (plan_ctx, None, fake), (plan_ctx, fake, None)):
        assert call_range(lib, *args) == INVALID_ARG
    assert call_range(lib, plan_ctx, fake, fake, out=False) == INVALID_ARG
    for bad in (dict(nby=-1), dict(nby=8), dict(nby=1, by=False), dict(lo_strict=-1), dict(lo_strict=2), dict(hi_strict=-1), dict(hi_strict=2),
                dict(join_type=-1), dict(join_type=4), dict(nleft_out=0, nright_out=0), dict(nleft_out=-1), dict(nright_out=-1), dict(outs=False),
                dict(join_type=SEMI), dict(join_type=ANTI), dict(join_type=SEMI, nleft_out=0), dict(join_type=ANTI, nleft_out=0, nright_out=0)):
        assert call_range(lib, plan_ctx, fake, fake, **bad) == INVALID_ARG, bad
        assert b"qe_result_range_join" in lib.qe_last_error(plan_ctx), bad


def test_the_stats_of_a_fresh_context(native_lib, plan_ctx):
    stats = (C.c_int64 * 4)(*[7] * 4)
    assert native_lib.qe_ctx_last_range_stats(plan_ctx, None) == INVALID_ARG and native_lib.qe_ctx_last_range_stats(None, stats) == INVALID_ARG
    assert native_lib.qe_ctx_last_range_stats(plan_ctx, stats) == N.OK and list(stats) == [0, 0, 0, 0]


# ---- the device path is taken only when both sources are GPU operators of one context ------------------------------------------
class FakeResult:
    ncols = 3

    def __init__(self, name):
        self.name, self.freed = name, False

    def free(self):
        self.freed = True


class FakeContext:
    """Records the one device call the operator makes."""

    def __init__(self):
        self.calls = []

    def range_join(self, lres, rres, *args):
        self.calls.append((lres.name, rres.name) + args)
        return FakeResult("out")


class FakeGpuSource:
    def __init__(self, ctx, name):
        self.ctx, self.name, self.opened = ctx, name, 0

    def open(self):
        self.opened += 1

    def close(self):
        pass

    def result(self):
        return FakeResult(self.name)


def test_the_operator_takes_the_device_path_only_for_gpu_sources_of_one_context():
    ctx = FakeContext()
    a, b = FakeGpuSource(ctx, "a"), FakeGpuSource(ctx, "b")
    op = RangeJoinOperator(a, b, [0], [1], 1, 2, 0, True, False, LEFT)
    assert isinstance(op, DeviceResultOperator) and op.ctx is ctx
    op.open()
    assert ctx.calls == [("a", "b", [0], [1], 1, 2, 0, True, False, LEFT, [0, 1, 2], [0, 1, 2])]   # every column of both sides
    assert op.result().name == "out"
    out = op.result()
    op.close()
    assert out.freed and (a.opened, b.opened) == (1, 1)
    ctx.calls.clear()
    op = RangeJoinOperator(a, a, [], [], 1, 1, 0, join_type=ANTI, left_out=[2])                    # one object on both sides: opened once
    op.open()
    assert ctx.calls == [("a", "a", [], [], 1, 1, 0, False, False, ANTI, [2], [])] and a.opened == 2
    op.close()
    ctx.calls.clear()
    op = RangeJoinOperator(a, b, [0], [0], 1, 2, 0, join_type=SEMI)                                # SEMI: every left column, no right column
    op.open()
    assert ctx.calls[0][-2:] == ([0, 1, 2], [])
    op.close()
    other = FakeGpuSource(FakeContext(), "c")
    rows = Rows([[1, 0, 5]])
    for left, right in ((a, other), (rows, b), (a, rows), (rows, rows)):
        op = RangeJoinOperator(left, right, [0], [0], 1, 2, 1)
        assert not hasattr(op, "ctx")
    ctx.calls.clear()
    assert op_map(RangeJoinOperator(rows, Rows([[1, 3]]), [0], [0], 1, 2, 1), list) == [[1, 0, 5, 1, 3]] and ctx.calls == []
