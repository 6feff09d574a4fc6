"""RIGHT and FULL OUTER joins without a GPU: the host branches of ``HashJoinOperator`` and ``RangeJoinOperator`` -- the
executable statement of the semantics -- against answers written out here, the numpy reference of the device tests
(tests/outer_join_reference.py) against those host branches row for row, the constructor errors, and what the C ABI decides
about the two new join types from its scalar arguments alone (a planning-only context and handles that are never dereferenced,
as in tests/test_range_join_cpu.py).

The output is a HEAD (the INNER rows for RIGHT, the LEFT rows for FULL) followed by a TAIL: every build / right row that no
probe / left row matched, once, in build / right row order, with ``None`` for every probe / left column."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

from queryengine_amd import Column, DataType
from queryengine_amd import native as N
from queryengine_amd.operators import AsofJoinOperator, HashJoinOperator, RangeJoinOperator, map as op_map

from outer_join_reference import FULL, HASH_PROBE, RANGE_JOIN, RIGHT, hash_outer_pairs, outer_expected, range_outer_pairs
from test_asof_cpu import call_asof
from test_range_join_cpu import STRICTS, call_range, random_case, rjoin
from test_setop_cpu import DICT_MODES, Rows, assert_rows, boxed, dictionaries, side_column

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
INNER, LEFT, SEMI, ANTI = N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI
NAN = float("nan")
NAN2 = struct.unpack("<d", struct.pack("<Q", 0x7ff8000000000002))[0]        # a NaN with a payload: the same key as NAN
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1


def hjoin(probe, build, pk, bk, jt, probe_out=None, build_out=None):
    return op_map(HashJoinOperator(Rows(probe), Rows(build), pk, bk, jt, probe_out, build_out), lambda r: list(r))


# ---- answers written out: the hash join ---------------------------------------------------------------------------------------------
def test_an_unmatched_build_row_in_the_middle():
    probe, build = [[1, "p0"], [3, "p1"], [9, "p2"]], [[1, "b0"], [2, "b1"], [3, "b2"]]
    assert hjoin(probe, build, [0], [0], RIGHT) == [[1, "p0", 1, "b0"], [3, "p1", 3, "b2"], [None, None, 2, "b1"]]
    assert hjoin(probe, build, [0], [0], FULL) == [[1, "p0", 1, "b0"], [3, "p1", 3, "b2"], [9, "p2", None, None], [None, None, 2, "b1"]]


def test_a_null_key_build_row_is_in_the_tail():
    probe, build = [[None, "p0"], [5, "p1"]], [[None, "b0"], [5, "b1"], [None, "b2"]]
    assert hjoin(probe, build, [0], [0], RIGHT, [1], [1]) == [["p1", "b1"], [None, "b0"], [None, "b2"]]
    assert hjoin(probe, build, [0], [0], FULL, [1], [1]) == [["p0", None], ["p1", "b1"], [None, "b0"], [None, "b2"]]


def test_a_build_row_matched_by_three_probe_rows_is_in_no_tail():
    probe, build = [[7, 0], [7, 1], [8, 2], [7, 3]], [[7, "b0"], [6, "b1"]]
    assert hjoin(probe, build, [0], [0], RIGHT, [1], [1]) == [[0, "b0"], [1, "b0"], [3, "b0"], [None, "b1"]]
    assert hjoin(probe, build, [0], [0], FULL, [1], [1]) == [[0, "b0"], [1, "b0"], [2, None], [3, "b0"], [None, "b1"]]


def test_duplicate_build_keys_all_matched():
    probe, build = [[4, "p0"]], [[4, "b0"], [4, "b1"], [4, "b0"]]                # two EQUAL build rows are two rows
    for jt in (RIGHT, FULL):
        assert hjoin(probe, build, [0], [0], jt, [1], [1]) == [["p0", "b0"], ["p0", "b1"], ["p0", "b0"]]
    assert hjoin([[5, "p0"]], build, [0], [0], RIGHT, [1], [1]) == [[None, "b0"], [None, "b1"], [None, "b0"]]
    assert hjoin([[5, "p0"]], build, [0], [0], FULL, [1], [1]) == [["p0", None], [None, "b0"], [None, "b1"], [None, "b0"]]


def test_empty_sides_of_the_hash_join():
    build = [[1, "b0"], [2, "b1"]]
    for jt in (RIGHT, FULL):
        assert hjoin([], [], [0], [0], jt) == [] and hjoin([], [], [0], [0], jt, [0], [0]) == []               # both sides empty
        assert hjoin([], build, [0], [0], jt, [1, 0], [1]) == [[None, None, "b0"], [None, None, "b1"]]         # the tail is the whole build side
        assert hjoin([], build, [0], [0], jt, [], [0]) == [[1], [2]]                                           # no probe column at all
        with pytest.raises(ValueError, match="probe_out"):
            hjoin([], build, [0], [0], jt)                                                                     # how many Nones?
    assert hjoin([[1, "p0"]], [], [0], [0], RIGHT) == [] and hjoin([[1, "p0"]], [], [0], [0], RIGHT, None, [0]) == []
    assert hjoin([[1, "p0"]], [], [0], [0], FULL, None, [1, 0]) == [[1, "p0", None, None]]                     # FULL is LEFT
    with pytest.raises(ValueError, match="build_out"):
        hjoin([[1, "p0"]], [], [0], [0], FULL)


def test_one_source_on_both_sides_of_the_hash_join():
    src = Rows([[1, 1], [2, 5], [None, 2], [5, 9]])                               # column 0 probes column 1
    got = op_map(HashJoinOperator(src, src, [0], [1], FULL, [0], [1]), list)
    assert got == [[1, 1], [2, 2], [None, None], [5, 5], [None, 9]] and src.opens == 1
    got = op_map(HashJoinOperator(src, src, [0], [1], RIGHT, [0], [0, 1]), list)
    assert got == [[1, 1, 1], [2, None, 2], [5, 2, 5], [None, 5, 9]]


# ---- answers written out: the range join --------------------------------------------------------------------------------------------
def test_two_overlapping_intervals_over_one_right_row():
    right = [[5, "r0"], [9, "r1"]]
    left = [[4, 6, "l0"], [5, 7, "l1"]]
    assert rjoin(left, right, [], [], 0, 1, 0, join_type=RIGHT, left_out=[2], right_out=[1]) == [["l0", "r0"], ["l1", "r0"], [None, "r1"]]
    assert rjoin(left, right, [], [], 0, 1, 0, join_type=FULL, left_out=[2], right_out=[1]) == [["l0", "r0"], ["l1", "r0"], [None, "r1"]]


def test_two_adjacent_half_open_intervals_leave_exactly_the_boundary_row_out():
    right = [[v, f"r{v}"] for v in (1, 2, 3, 4, 5)]
    left = [[1, 3, "l0"], [3, 5, "l1"]]
    ids = lambda ls, hs, jt: [r[-1] for r in rjoin(left, right, [], [], 0, 1, 0, ls, hs, jt, [2], [1]) if r[0] is None]   # noqa: E731
    for jt in (RIGHT, FULL):
        assert ids(False, True, jt) == ["r5"]                                     # [1, 3) and [3, 5): nothing between them is left out
        assert ids(True, True, jt) == ["r1", "r3", "r5"]                          # (1, 3) and (3, 5): exactly the boundary (and the two ends)
        assert ids(False, False, jt) == []
    assert rjoin(left, right, [], [], 0, 1, 0, True, True, RIGHT, [2], [1]) == [["l0", "r2"], ["l1", "r4"], [None, "r1"], [None, "r3"], [None, "r5"]]


def test_an_empty_interval_and_a_null_on():
    right = [["k", 2, "r0"], ["k", None, "r1"], [None, 2, "r2"], ["k", 3, "r3"]]          # by, on, name
    left = [["k", 3, 1, "l0"], ["k", 3, 3, "l1"]]                                         # l0: a reversed, empty interval
    assert rjoin(left, right, [0], [0], 1, 2, 1, join_type=RIGHT, left_out=[3], right_out=[2]) == [
        ["l1", "r3"], [None, "r0"], [None, "r1"], [None, "r2"]]                            # the NULL on and the NULL by never match
    assert rjoin(left, right, [0], [0], 1, 2, 1, join_type=FULL, left_out=[3], right_out=[2]) == [
        ["l0", None], ["l1", "r3"], [None, "r0"], [None, "r1"], [None, "r2"]]


def test_empty_sides_of_the_range_join():
    right = [[1, "r0"], [2, "r1"]]
    for jt in (RIGHT, FULL):
        assert rjoin([], [], [], [], 0, 1, 0, join_type=jt) == []
        assert rjoin([], right, [], [], 0, 1, 0, join_type=jt, left_out=[0], right_out=[1]) == [[None, "r0"], [None, "r1"]]
        with pytest.raises(ValueError, match="left_out"):
            rjoin([], right, [], [], 0, 1, 0, join_type=jt)
    assert rjoin([[1, 2]], [], [], [], 0, 1, 0, join_type=RIGHT) == []
    assert rjoin([[1, 2]], [], [], [], 0, 1, 0, join_type=FULL, right_out=[0]) == [[1, 2, None]]
    with pytest.raises(ValueError, match="right_out"):
        rjoin([[1, 2]], [], [], [], 0, 1, 0, join_type=FULL)


def test_one_source_on_both_sides_of_the_range_join():
    src = Rows([[1, 10, 30], [2, 20, 20], [1, 30, 10], [1, 30, 10]])              # by, lo (and on), hi; the last two rows are equal
    got = op_map(RangeJoinOperator(src, src, [0], [0], 1, 2, 1, False, False, RIGHT, [1], [1]), list)
    assert got == [[10, 10], [10, 30], [10, 30], [20, 20]] and src.opens == 1
    got = op_map(RangeJoinOperator(src, src, [0], [0], 1, 2, 1, True, False, FULL, [1], [1, 2]), list)
    assert got == [[10, 30, 10], [10, 30, 10], [20, None, None], [30, None, None], [30, None, None], [None, 10, 30], [None, 20, 20]]


# ---- the numpy reference equals the host branches -----------------------------------------------------------------------------------
KEY_POOLS = {D: [NAN, NAN2, -0.0, 0.0, 1.5, -2.25], I64: [2 ** 53, 2 ** 53 + 1, -(2 ** 63), 0, 7], I32: [0, -1, 2 ** 31 - 1, 5], B: [False, True]}
TAGS = ["t0", "", "täg"]
OUTS = [[0], [0, 1], [1, 0, 0], [], [2, 0]]         # of (row id, tag, first key column)


def expected_rows(want):
    return boxed([Column(w.type, w.data, w.valid, w.dictionary) for w in want], len(want[0].data))


def check_nones(want, lrow, rrow, nleft_out):
    """The value under a none is zero and its validity 0, on BOTH sides."""
    for k, w in enumerate(want):
        none = (lrow if k < nleft_out else rrow) < 0
        assert np.array_equal(w.zero_at, none) and not (w.valid & none).any() and not w.data[none].any()


def random_hash_case(seed):
    """Both sides draw their key tuples from one small pool, so that duplicate keys meet across the sides and some build keys
    meet nothing.  Columns of a side: the key columns, then row id, tag, a DOUBLE."""
    rng = np.random.default_rng(seed)
    nkeys = int(rng.integers(1, 5))
    types = [[D, I64, I32, B, S][i] for i in rng.integers(0, 5, nkeys)]
    types[int(rng.integers(0, nkeys))] = [D, I64, I32, B, S][seed % 5]
    dicts = [dictionaries(rng, DICT_MODES[int(rng.integers(0, len(DICT_MODES)))]) if t == S else (None, None) for t in types]
    tuples = []
    for _ in range(int(rng.integers(1, 7))):
        row = []
        for t, (pd, bd) in zip(types, dicts):
            pool = pd + bd if t == S else KEY_POOLS[t]
            row.append(None if rng.random() < 0.1 else pool[int(rng.integers(0, len(pool)))])
        tuples.append(row)
    sides = []
    for which in (0, 1):
        n = int(rng.integers(0, 41))
        picks = rng.integers(0, len(tuples), n)
        keys = [side_column(t, rng, [tuples[i][c] for i in picks], rng.random() < 0.6, dicts[c][which]) for c, t in enumerate(types)]
        value = np.where(rng.random(n) < 0.2, np.array([NAN2, -0.0])[rng.integers(0, 2, n)], rng.integers(-9, 9, n).astype(np.float64))
        sides.append(keys + [Column(I64, np.arange(n, dtype=np.int64)),
                             Column(S, rng.integers(0, len(TAGS), n).astype(np.int32), (rng.random(n) > 0.3) if n else None, TAGS), Column(D, value)])
    outs = [[[nkeys, nkeys + 1, 0][c] for c in OUTS[int(rng.integers(0, len(OUTS)))]] for _ in (0, 1)]
    if not outs[0] and not outs[1]:
        outs[1] = [nkeys]
    return sides[0], sides[1], list(range(nkeys)), outs[0], outs[1], types


@pytest.mark.parametrize("block", range(8))
def test_the_hash_reference_equals_the_host_branch(block):
    """320 seeded inputs of at most 40 rows a side, RIGHT and FULL each: 1 to 4 key columns of all five types, each nullable or
    not, NaN with and without a payload, -0.0 and 0.0, every dictionary mode; either output list may be empty."""
    seen, tails, matched = set(), 0, 0
    for seed in range(block * 40, block * 40 + 40):
        pcols, bcols, keys, probe_out, build_out, types = random_hash_case(seed)
        seen |= set(types)
        prows, brows = boxed(pcols, len(pcols[0])), boxed(bcols, len(bcols[0]))
        for jt in (RIGHT, FULL):
            prow, brow, stats = hash_outer_pairs(pcols, bcols, keys, keys, jt)
            want = outer_expected(pcols, bcols, [c.valid is not None for c in bcols], prow, brow, probe_out, build_out, jt)
            got = hjoin(prows, brows, keys, keys, jt, probe_out, build_out)
            assert_rows(got, expected_rows(want), f"seed {seed} join {jt}")
            head = hjoin(prows, brows, keys, keys, INNER if jt == RIGHT else LEFT, probe_out, build_out)
            assert_rows(got[:len(head)], head, f"seed {seed} join {jt}: the head")
            assert stats == [HASH_PROBE, len(head), len(got) - len(head), len(brows) - (len(got) - len(head))]
            assert np.array_equal(brow[stats[1]:], np.sort(brow[stats[1]:])) and (prow[stats[1]:] == -1).all() and (prow[:stats[1]] >= 0).all()
            assert [w.nullable for w in want] == [True] * len(probe_out) + [jt == FULL or bcols[c].valid is not None for c in build_out]
            check_nones(want, prow, brow, len(probe_out))
            tails += stats[2]
            matched += stats[3]
    assert seen == {D, I64, I32, B, S} and tails > 200 and matched > 200


@pytest.mark.parametrize("block", range(8))
def test_the_range_reference_equals_the_host_branch(block):
    """200 seeded inputs of tests/test_range_join_cpu.py (at most 40 rows a side; every value type, all five by types, 0 to 7 by
    columns, every dictionary mode, NaN / +-0.0 / +-Inf, lo and hi as one column), RIGHT and FULL under the four strict
    combinations each."""
    tails, matched = 0, 0
    for seed in range(block * 25, block * 25 + 25):
        q = random_case(seed)
        left, right = q["left"], q["right"]
        lrows, rrows = boxed(left, len(left[0])), boxed(right, len(right[0]))
        for jt in (RIGHT, FULL):
            for lo_strict, hi_strict in STRICTS:
                args = (q["left_by"], q["right_by"], q["lo"], q["hi"], q["on"], lo_strict, hi_strict)
                lrow, rrow, stats, _ = range_outer_pairs(left, right, *args, jt)
                want = outer_expected(left, right, [c.valid is not None for c in right], lrow, rrow, q["left_out"], q["right_out"], jt)
                got = rjoin(lrows, rrows, *args, jt, q["left_out"], q["right_out"])
                assert_rows(got, expected_rows(want), f"seed {seed} join {jt} strict {lo_strict} {hi_strict}")
                head = rjoin(lrows, rrows, *args, INNER if jt == RIGHT else LEFT, q["left_out"], q["right_out"])
                assert_rows(got[:len(head)], head, f"seed {seed} join {jt}: the head")
                assert stats == [RANGE_JOIN, len(head), len(got) - len(head), len(rrows) - (len(got) - len(head))]
                assert [w.nullable for w in want] == [True] * len(q["left_out"]) + [jt == FULL or right[c].valid is not None for c in q["right_out"]]
                check_nones(want, lrow, rrow, len(q["left_out"]))
                tails += stats[2]
                matched += stats[3]
    assert tails > 200 and matched > 100


# ---- constructor errors -------------------------------------------------------------------------------------------------------------
def test_join_types_of_the_operators():
    for bad in (4, 5, 6, 7, 10, -1, True, None):
        with pytest.raises(ValueError, match="unknown join type"):
            HashJoinOperator(Rows([]), Rows([]), [0], [0], bad)
        with pytest.raises(ValueError, match="unknown join type"):
            RangeJoinOperator(Rows([]), Rows([]), [0], [0], 1, 2, 1, join_type=bad)
    for bad in (RIGHT, FULL, SEMI, ANTI, 4, True, None):
        with pytest.raises(ValueError, match="the join type is INNER or LEFT"):
            AsofJoinOperator(Rows([]), Rows([]), [0], [0], 1, 1, join_type=bad)
    for jt in (RIGHT, FULL):
        assert HashJoinOperator(Rows([]), Rows([]), [0], [0], jt).join_type == jt
        assert RangeJoinOperator(Rows([]), Rows([]), [0], [0], 1, 2, 1, join_type=jt).join_type == jt
        HashJoinOperator(Rows([]), Rows([]), [0], [0], jt, [], [0])                     # RIGHT with no probe column is legal
        HashJoinOperator(Rows([]), Rows([]), [0], [0], jt, [], None)
        with pytest.raises(ValueError, match="no output column"):
            HashJoinOperator(Rows([]), Rows([]), [0], [0], jt, [], [])
        with pytest.raises(ValueError, match="no output column"):
            RangeJoinOperator(Rows([]), Rows([]), [0], [0], 1, 2, 1, join_type=jt, left_out=[], right_out=[])


# ---- the C ABI on a planning-only context -------------------------------------------------------------------------------------------
@pytest.fixture()
def plan_ctx(native_lib):
    ctx = C.c_void_p()
    assert native_lib.qe_ctx_create(N.DEVICE_NONE, None, C.byref(ctx)) == N.OK
    yield ctx
    native_lib.qe_ctx_destroy(ctx)


def test_the_abi_takes_the_two_types_where_it_should(native_lib, plan_ctx):
    lib = native_lib
    fake = C.c_void_p(0x1000)           # never dereferenced: every check below comes before the first look at a result
    for jt in (RIGHT, FULL):            # accepted: the NEXT check of the scalar arguments is the one that fails
        assert call_range(lib, plan_ctx, fake, fake, join_type=jt, nleft_out=0, nright_out=0) == INVALID_ARG
        assert b"no output column" in lib.qe_last_error(plan_ctx), lib.qe_last_error(plan_ctx)
        assert call_asof(lib, plan_ctx, fake, fake, join_type=jt) == INVALID_ARG
        assert b"the join type is INNER or LEFT" in lib.qe_last_error(plan_ctx)
    for jt in (4, 5, 6, 7, 10, 40, -1):
        assert call_range(lib, plan_ctx, fake, fake, join_type=jt, nleft_out=0, nright_out=0) == INVALID_ARG
        assert b"unknown join type" in lib.qe_last_error(plan_ctx), jt


def test_the_outer_stats_of_a_fresh_context(native_lib, plan_ctx):
    stats = (C.c_int64 * 4)(*[7] * 4)
    assert native_lib.qe_ctx_last_outer_stats(plan_ctx, None) == INVALID_ARG and native_lib.qe_ctx_last_outer_stats(None, stats) == INVALID_ARG
    assert native_lib.qe_ctx_last_outer_stats(plan_ctx, stats) == N.OK and list(stats) == [0, 0, 0, 0]


def test_constants():
    assert (N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI) == (0, 1, 2, 3) and (N.JOIN_RIGHT, N.JOIN_FULL) == (8, 9)
    header = open(os.path.join(ROOT, "include", "qe_hip.h")).read()
    assert re.search(r"QE_JOIN_ANTI\s*=\s*3\s*,\s*QE_JOIN_RIGHT\s*=\s*8\s*,\s*QE_JOIN_FULL\s*=\s*9\s*}", header)
