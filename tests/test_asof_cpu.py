"""The ASOF join without a GPU: the host branch of ``AsofJoinOperator`` against answers written out here, the numpy reference
of the device tests (tests/asof_reference.py) against that host branch row for row, and the argument checks of the Python
layer and of qe_result_asof_join that need no device.

A planning-only context cannot hold a result, so the ABI is reached here with handles that are never dereferenced: the null
pointers and every error that qe_result_asof_join decides from its scalar arguments alone (nby, direction, strict, join_type,
the column counts).  The errors that need a result to look at -- a column out of range, paired by columns of different types,
the type of the `on` column -- are in tests/test_gpu_asof.py.  Not tested anywhere: QE_ERR_HIP on a planning-only context
(it would need a result there), a STRING by column without a dictionary (the ABI cannot build one)."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from queryengine_amd import Column, DataType
from queryengine_amd import native as N
from queryengine_amd.operators import AsofJoinOperator, map as op_map

from asof_reference import asof_reference
from test_setop_cpu import NPTYPE, POOLS, Rows, assert_rows, boxed, dictionaries, side_column, DICT_MODES

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
BACK, FWD = N.ASOF_BACKWARD, N.ASOF_FORWARD
INNER, LEFT = N.JOIN_INNER, N.JOIN_LEFT
FORMS = [(d, s, j) for d in (BACK, FWD) for s in (False, True) for j in (INNER, LEFT)]
NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1


def asof(left, right, left_by, right_by, left_on, right_on, direction=BACK, strict=False, join_type=LEFT, left_out=None, right_out=None):
    return op_map(AsofJoinOperator(Rows(left), Rows(right), left_by, right_by, left_on, right_on, direction, strict, join_type,
                                   left_out, right_out), lambda r: list(r))


# ---- answers written out ---------------------------------------------------------------------------------------------------------
def test_trades_and_quotes():
    quotes = [["a", 1, 10.0], ["b", 2, 20.0], ["a", 3, 11.0], ["a", 7, 12.0], ["b", 9, 21.0]]      # symbol, time, price
    trades = [["a", 2], ["b", 1], ["a", 7], ["c", 5], ["b", 100]]
    assert_rows(asof(trades, quotes, [0], [0], 1, 1, right_out=[1, 2]),
                [["a", 2, 1, 10.0], ["b", 1, None, None], ["a", 7, 7, 12.0], ["c", 5, None, None], ["b", 100, 9, 21.0]])
    assert_rows(asof(trades, quotes, [0], [0], 1, 1, strict=True, right_out=[1, 2]),
                [["a", 2, 1, 10.0], ["b", 1, None, None], ["a", 7, 3, 11.0], ["c", 5, None, None], ["b", 100, 9, 21.0]])
    assert_rows(asof(trades, quotes, [0], [0], 1, 1, FWD, right_out=[1, 2]),
                [["a", 2, 3, 11.0], ["b", 1, 2, 20.0], ["a", 7, 7, 12.0], ["c", 5, None, None], ["b", 100, None, None]])
    assert_rows(asof(trades, quotes, [0], [0], 1, 1, FWD, True, INNER, right_out=[1]), [["a", 2, 3], ["b", 1, 2]])
    assert_rows(asof(trades, quotes, [], [], 1, 1, right_out=[0, 1]),                                # no by column: one partition
                [["a", 2, "b", 2], ["b", 1, "a", 1], ["a", 7, "a", 7], ["c", 5, "a", 3], ["b", 100, "b", 9]])


def test_ties_go_to_the_last_right_row_backward_and_to_the_first_forward():
    right = [[1, 0], [2, 1], [2, 2], [2, 3], [3, 4]]                                                # on, row id
    left = [[2], [2], [0], [4]]
    assert asof(left, right, [], [], 0, 0, BACK, False, right_out=[1]) == [[2, 3], [2, 3], [0, None], [4, 4]]
    assert asof(left, right, [], [], 0, 0, BACK, True, right_out=[1]) == [[2, 0], [2, 0], [0, None], [4, 4]]
    assert asof(left, right, [], [], 0, 0, FWD, False, right_out=[1]) == [[2, 1], [2, 1], [0, 0], [4, None]]
    assert asof(left, right, [], [], 0, 0, FWD, True, right_out=[1]) == [[2, 4], [2, 4], [0, 0], [4, None]]


def test_special_values_of_on():
    def rid(left_on, right_ons, direction, strict):
        got = asof([[left_on]], [[v, i] for i, v in enumerate(right_ons)], [], [], 0, 0, direction, strict, right_out=[1])
        return got[0][1]
    assert rid(0.0, [-0.0], BACK, True) == 0 and rid(-0.0, [0.0], BACK, False) is None               # -0.0 < 0.0
    assert rid(-0.0, [0.0], FWD, True) == 0 and rid(0.0, [-0.0], FWD, False) is None
    assert rid(NAN, [INF, NAN, NAN], BACK, False) == 2 and rid(NAN, [INF, NAN, NAN], BACK, True) == 0  # all NaNs equal, above +Inf
    assert rid(NAN, [NAN, NAN], FWD, False) == 0 and rid(NAN, [NAN, 1.0], FWD, True) is None
    assert rid(INF, [NAN], FWD, True) == 0 and rid(-INF, [NAN, -INF], BACK, False) == 1
    big = 2 ** 53
    assert float(big) == float(big + 1)
    assert rid(big, [big + 1], BACK, False) is None and rid(big, [big + 1], FWD, True) == 0            # never through a double
    assert rid(big + 1, [big], BACK, True) == 0 and rid(2 ** 63 - 1, [-(2 ** 63)], BACK, False) == 0
    assert rid(-(2 ** 63), [2 ** 63 - 1], BACK, False) is None


def test_a_null_matches_nothing_and_hides_nothing():
    right = [["k", 1, 0], ["k", None, 1], [None, 2, 2], ["k", 3, 3]]                                 # by, on, row id
    assert asof([["k", 2]], right, [0], [0], 1, 1, BACK, right_out=[2]) == [["k", 2, 0]]               # not the NULL on, nor past it
    assert asof([["k", None]], right, [0], [0], 1, 1, FWD, right_out=[2]) == [["k", None, None]]       # NULL sorts first: still nothing
    assert asof([["k", None]], right, [0], [0], 1, 1, BACK, right_out=[2]) == [["k", None, None]]
    assert asof([[None, 2]], right, [0], [0], 1, 1, BACK, right_out=[2]) == [[None, 2, None]]          # NULL by on both sides
    assert asof([[None, 2], ["k", 9]], right, [0], [0], 1, 1, BACK, join_type=INNER, right_out=[2]) == [["k", 9, 3]]


def test_by_keys_compare_like_join_keys_and_never_leak():
    nan2 = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000002))[0]
    right = [[NAN, 1, 0], [0.0, 1, 1], [-0.0, 5, 2]]
    left = [[nan2, 2], [-0.0, 2], [0.0, 2], [1.5, 2]]
    assert [r[2] for r in asof(left, right, [0], [0], 1, 1, BACK, right_out=[2])] == [0, None, 1, None]
    assert [r[2] for r in asof(left, right, [0], [0], 1, 1, FWD, right_out=[2])] == [None, 2, None, None]
    same = [[1, 10], [2, 20], [1, 30]]                                                               # a source against itself
    src = Rows(same)
    got = op_map(AsofJoinOperator(src, src, [0], [0], 1, 1, BACK, True, LEFT, [1], [1]), list)
    assert got == [[10, None], [20, None], [30, 10]] and src.opens == 1
    got = op_map(AsofJoinOperator(src, src, [0], [0], 1, 1, BACK, False, LEFT, [1], [1]), list)
    assert got == [[10, 10], [20, 20], [30, 30]]


# ---- the numpy reference equals the host branch ---------------------------------------------------------------------------------
ON_POOLS = {D: [NAN, -0.0, 0.0, INF, -INF, 1.5, -2.25], I64: [2 ** 53, 2 ** 53 + 1, -(2 ** 63), 2 ** 63 - 1, 0, 7], I32: [0, -1, 2 ** 31 - 1, -(2 ** 31), 5]}
TAGS = ["t0", "", "täg"]
OUTS = [[0], [0, 1], [1, 0, 0], [], [2, 0]]         # of (row id, tag, on)


def random_case(seed):
    """Both sides draw their by tuples from one small pool and their `on` from a pool of special values, so that partitions and
    equal `on` values meet across the sides.  Left columns: by.., on, row id, tag; right columns: row id, tag, on, by.."""
    rng = np.random.default_rng(seed)
    nby = [0, 1, 1, 2, 3, 7][int(rng.integers(0, 6))]
    types = [[D, I64, I32, B, S][i] for i in rng.integers(0, 5, nby)]
    if nby:
        types[int(rng.integers(0, nby))] = [D, I64, I32, B, S][seed % 5]
    on_type = [D, I64, I32][(seed // 5) % 3]
    dicts = [dictionaries(rng, DICT_MODES[int(rng.integers(0, len(DICT_MODES)))]) if t == S else (None, None) for t in types]
    tuples = []
    for _ in range(int(rng.integers(1, 5))):
        row = []
        for t, (ld, rd) in zip(types, dicts):
            pool = ld + rd if t == S else POOLS[t]
            row.append(None if rng.random() < 0.12 else pool[int(rng.integers(0, len(pool)))])
        tuples.append(row)
    sides = []
    for which in (0, 1):
        n = int(rng.integers(0, 41))
        picks = rng.integers(0, len(tuples), n)
        by = [side_column(t, rng, [tuples[i][c] for i in picks], rng.random() < 0.5, dicts[c][which]) for c, t in enumerate(types)]
        pool = ON_POOLS[on_type]
        ons = [None if rng.random() < 0.15 else pool[int(rng.integers(0, len(pool)))] for _ in range(n)]
        on = side_column(on_type, rng, ons, rng.random() < 0.6, None)
        rowid = Column(I64, np.arange(n, dtype=np.int64))
        tag = Column(S, rng.integers(0, len(TAGS), n).astype(np.int32), (rng.random(n) > 0.3) if n else None, TAGS)
        sides.append(by + [on, rowid, tag] if which == 0 else [rowid, tag, on] + by)
    left_out = [[nby + 1, nby + 2, nby][c] for c in OUTS[int(rng.integers(0, len(OUTS)))]]
    right_out = [[0, 1, 2][c] for c in OUTS[int(rng.integers(0, len(OUTS)))]]
    if not left_out and not right_out:
        right_out = [0]
    return dict(left=sides[0], right=sides[1], left_by=list(range(nby)), right_by=list(range(3, 3 + nby)), left_on=nby, right_on=2,
                left_out=left_out, right_out=right_out, on_type=on_type, types=types)


@pytest.mark.parametrize("block", range(8))
def test_the_numpy_reference_equals_the_host_branch(block):
    """360 seeded inputs of at most 40 rows a side, all eight forms each: every `on` type, all five by types, 0 to 7 by columns,
    each column nullable or not, every dictionary mode, NaN / +-0.0 / +-Inf and INT64 values that differ only beyond 2^53."""
    seen_by, seen_on, matched, unmatched = set(), set(), 0, 0
    for seed in range(block * 45, block * 45 + 45):
        q = random_case(seed)
        left, right = q["left"], q["right"]
        seen_by |= set(q["types"])
        seen_on.add(q["on_type"])
        lrows, rrows = boxed(left, len(left[0])), boxed(right, len(right[0]))
        for direction, strict, join_type in FORMS:
            want, stats = asof_reference(left, right, [c.valid is not None for c in left], [c.valid is not None for c in right], q["left_by"],
                                         q["right_by"], q["left_on"], q["right_on"], direction, strict, join_type, q["left_out"], q["right_out"])
            rows = boxed([Column(w.type, w.data, w.valid, w.dictionary) for w in want], len(want[0].data))
            got = asof(lrows, rrows, q["left_by"], q["right_by"], q["left_on"], q["right_on"], direction, strict, join_type,
                       q["left_out"], q["right_out"])
            assert_rows(got, rows, f"seed {seed} direction {direction} strict {strict} join {join_type}")
            assert len(got) == (stats["matched"] if join_type == INNER else len(lrows))
            assert [w.nullable for w in want] == [left[c].valid is not None for c in q["left_out"]] + \
                [right[c].valid is not None or join_type == LEFT for c in q["right_out"]]
            for w in want[len(q["left_out"]):]:
                assert w.zero_at is not None and not (w.valid & w.zero_at).any() and not w.data[w.zero_at].any()
            assert (stats["left_rows"], stats["right_rows"]) == (len(lrows), len(rrows))
            matched += stats["matched"]
            unmatched += len(lrows) - stats["matched"]
    assert seen_by == {D, I64, I32, B, S} and seen_on == {D, I64, I32} and matched > 100 and unmatched > 100


def test_the_partition_count_of_the_reference():
    left = [Column(I32, np.array([1, 1, 2], dtype=np.int32), np.array([True, False, True])), Column(I32, np.arange(3, dtype=np.int32))]
    right = [Column(I32, np.array([2, 3, 9], dtype=np.int32), np.array([True, True, False])), Column(I32, np.arange(3, dtype=np.int32))]
    _, stats = asof_reference(left, right, [True, False], [True, False], [0], [0], 1, 1, BACK, False, LEFT, [1], [1])
    assert stats == {"left_rows": 3, "right_rows": 3, "matched": 1, "partitions": 4}                  # NULL, 1, 2, 3: NULL is one value
    _, stats = asof_reference(left, right, [True, False], [True, False], [], [], 1, 1, BACK, False, LEFT, [1], [1])
    assert stats["partitions"] == 1 and stats["matched"] == 3
    none = [Column(I32, np.zeros(0, dtype=np.int32))]
    want, stats = asof_reference(none, none, [False], [False], [], [], 0, 0, FWD, True, LEFT, [0], [0])
    assert stats == {"left_rows": 0, "right_rows": 0, "matched": 0, "partitions": 0} and [w.nullable for w in want] == [False, True]


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_of_the_operator():
    ok = dict(left_by=[0], right_by=[0], left_on=1, right_on=1)
    for bad in (dict(direction=2), dict(direction=-1), dict(direction=None), dict(direction=True), dict(strict=2), dict(strict=None),
                dict(join_type=N.JOIN_SEMI), dict(join_type=N.JOIN_ANTI), dict(join_type=None), dict(left_by=[0, 1]), dict(left_by=list(range(8)),
                right_by=list(range(8))), dict(left_out=[], right_out=[])):
        with pytest.raises(ValueError):
            AsofJoinOperator(Rows([]), Rows([]), **{**ok, **bad})
    for left, right in ((None, Rows([])), (Rows([]), None)):
        with pytest.raises(ValueError):
            AsofJoinOperator(left, right, **ok)
    with pytest.raises(ValueError):
        asof([[1, "x"]], [[1, "y"]], [0], [0], 1, 1)                               # an `on` column that is not numeric
    with pytest.raises(ValueError):
        asof([[1, True]], [[1, True]], [0], [0], 1, 1)
    with pytest.raises(ValueError):
        asof([[1, 2]], [[1, 2.0]], [0], [0], 1, 1)                                 # whose type differs between the sides
    with pytest.raises(ValueError):
        asof([[1, 2]], [], [0], [0], 1, 1)                                         # LEFT, no right row, right_out not given
    assert asof([[1, 2]], [], [0], [0], 1, 1, right_out=[0, 1]) == [[1, 2, None, None]]
    assert asof([[1, 2]], [], [0], [0], 1, 1, join_type=INNER) == [] and asof([], [[1, 2]], [0], [0], 1, 1) == []


def test_constants_of_the_python_layer():
    assert (N.ASOF_BACKWARD, N.ASOF_FORWARD) == (0, 1)
    text = open(os.path.join(ROOT, "queryengine_amd", "csrc", "qe_kernels.h")).read()
    assert N.ASOF_BLOCKS == int(re.search(r"constexpr\s+int\s+kAsofBlocks\s*=\s*(\d+)\s*;", text).group(1))
    kernels = open(os.path.join(ROOT, "queryengine_amd", "csrc", "qe_asof.hip")).read()
    assert "dim3(256)" in kernels and "dim3(128)" not in kernels and "dim3(512)" not in kernels     # ASOF_BLOCKS counts blocks of 256 lanes
    header = open(os.path.join(ROOT, "include", "qe_hip.h")).read()
    assert re.search(r"QE_ASOF_BACKWARD\s*=\s*0\s*,\s*QE_ASOF_FORWARD\s*=\s*1", header)


@pytest.fixture()
def plan_ctx(native_lib):
    """A planning-only context: no device, so no result can live on it."""
    ctx = C.c_void_p()
    assert native_lib.qe_ctx_create(N.DEVICE_NONE, None, C.byref(ctx)) == N.OK
    yield ctx
    native_lib.qe_ctx_destroy(ctx)


def call_asof(lib, ctx, left, right, nby=1, direction=0, strict=0, join_type=LEFT, nleft_out=1, nright_out=1, by=True, outs=True, out=True):
    cols = (C.c_int32 * 8)(*range(8))
    res = C.c_void_p(0xdead)
    st = lib.qe_result_asof_join(ctx, left, right, cols if by else None, cols if by else None, nby, 0, 0, direction, strict, join_type,
                                 cols if outs else None, nleft_out, cols if outs else None, nright_out, C.byref(res) if out else None)
    if out:
        assert res.value is None, "*out must be NULL after an error"
    return st


def test_errors_that_need_no_result(native_lib, plan_ctx):
    lib = native_lib
    fake = C.c_void_p(0x1000)           # never dereferenced: every check below comes before the first look at a result
    for args in ((None, fake, fake), (plan_ctx, None, fake), (plan_ctx, fake, None)):
        assert call_asof(lib, *args) == INVALID_ARG
    assert call_asof(lib, plan_ctx, fake, fake, out=False) == INVALID_ARG
    for bad in (dict(nby=-1), dict(nby=8), dict(nby=1, by=False), dict(direction=-1), dict(direction=2), dict(strict=-1), dict(strict=2),
                dict(join_type=N.JOIN_SEMI), dict(join_type=N.JOIN_ANTI), dict(join_type=-1), dict(join_type=4),
                dict(nleft_out=0, nright_out=0), dict(nleft_out=-1), dict(nright_out=-1), dict(outs=False)):
        assert call_asof(lib, plan_ctx, fake, fake, **bad) == INVALID_ARG, bad
        assert b"qe_result_asof_join" in lib.qe_last_error(plan_ctx), bad


def test_the_stats_of_a_fresh_context(native_lib, plan_ctx):
    stats = (C.c_int64 * 4)(*[7] * 4)
    assert native_lib.qe_ctx_last_asof_stats(plan_ctx, None) == INVALID_ARG and native_lib.qe_ctx_last_asof_stats(None, stats) == INVALID_ARG
    assert native_lib.qe_ctx_last_asof_stats(plan_ctx, stats) == N.OK and list(stats) == [0, 0, 0, 0]
