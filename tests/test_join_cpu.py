"""The hash equi-join without a device: the host branch of ``HashJoinOperator`` -- the executable statement of the join's
semantics and the expectation of tests/test_gpu_join.py -- against hand-written row lists, and the argument checks of
qe_join_build that need no device (a planning-only context)."""
import ctypes as C

import numpy as np
import pytest

from queryengine_amd import Column, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N
from queryengine_amd.operators import HashJoinOperator, Operator, map as op_map

INNER, LEFT, SEMI, ANTI = N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI
NAN = float("nan")
INVALID_ARG, HIP = 1, 3


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


def join(probe, build, pk, bk, jt, probe_out=None, build_out=None):
    return op_map(HashJoinOperator(Rows(probe), Rows(build), pk, bk, jt, probe_out, build_out), lambda r: list(r))


def same(a, b):
    """Row lists equal, NaN equal to NaN and -0.0 different from 0.0."""
    return repr(a) == repr(b)


def test_duplicate_keys_on_both_sides_come_in_nested_loop_order():
    probe = [[1, "p0"], [2, "p1"], [1, "p2"], [3, "p3"]]
    build = [[2, "b0"], [1, "b1"], [1, "b2"], [4, "b3"], [2, "b4"]]
    assert join(probe, build, [0], [0], INNER) == [
        [1, "p0", 1, "b1"], [1, "p0", 1, "b2"], [2, "p1", 2, "b0"], [2, "p1", 2, "b4"], [1, "p2", 1, "b1"], [1, "p2", 1, "b2"]]
    assert join(probe, build, [0], [0], LEFT, [1], [1]) == [
        ["p0", "b1"], ["p0", "b2"], ["p1", "b0"], ["p1", "b4"], ["p2", "b1"], ["p2", "b2"], ["p3", None]]
    assert join(probe, build, [0], [0], SEMI, [1]) == [["p0"], ["p1"], ["p2"]]
    assert join(probe, build, [0], [0], ANTI, [1]) == [["p3"]]


def test_a_null_key_matches_nothing_on_either_side():
    probe = [[None, 0], [5, 1], [7, 2]]
    build = [[None, 10], [5, 11], [None, 12]]
    assert join(probe, build, [0], [0], INNER, [1], [1]) == [[1, 11]]
    assert join(probe, build, [0], [0], LEFT, [1], [1]) == [[0, None], [1, 11], [2, None]]
    assert join(probe, build, [0], [0], SEMI, [1]) == [[1]]
    assert join(probe, build, [0], [0], ANTI, [1]) == [[0], [2]]            # the NULL key counts as no match


def test_nan_is_one_value_and_the_zeros_are_two():
    other_nan = float(np.frombuffer(np.uint64(0xfff8000000000123).tobytes(), dtype=np.float64)[0])
    probe = [[NAN, 0], [0.0, 1], [-0.0, 2], [1.5, 3]]
    build = [[-0.0, 10], [other_nan, 11], [0.0, 12], [NAN, 13]]
    assert join(probe, build, [0], [0], INNER, [1], [1]) == [[0, 11], [0, 13], [1, 12], [2, 10]]
    assert join(probe, build, [0], [0], ANTI, [1]) == [[3]]
    got = join(probe, build, [0], [0], LEFT, [0, 1], [0])
    assert same(got, [[NAN, 0, other_nan], [NAN, 0, NAN], [0.0, 1, 0.0], [-0.0, 2, -0.0], [1.5, 3, None]])


def test_two_column_keys_pair_by_position():
    probe = [["a", True, 0], ["a", False, 1], ["b", None, 2], [None, True, 3]]
    build = [[False, "a", 10], [True, "a", 11], [True, "b", 12], [True, None, 13], [False, "a", 14]]
    assert join(probe, build, [0, 1], [1, 0], INNER, [2], [2]) == [[0, 11], [1, 10], [1, 14]]
    assert join(probe, build, [0, 1], [1, 0], LEFT, [2], [2]) == [[0, 11], [1, 10], [1, 14], [2, None], [3, None]]
    assert join(probe, build, [0, 1], [1, 0], SEMI, [2]) == [[0], [1]]
    assert join(probe, build, [0, 1], [1, 0], ANTI, [2]) == [[2], [3]]


def test_an_empty_side():
    rows = [[1, "x"], [2, "y"]]
    for jt, want in ((INNER, []), (LEFT, [[1, None], [2, None]]), (SEMI, []), (ANTI, [[1], [2]])):
        pairs = jt in (INNER, LEFT)
        assert join(rows, [], [0], [0], jt, [0], [1] if pairs else None) == want                  # empty build side
        assert join([], rows, [0], [0], jt, [0], [1] if pairs else None) == []                    # empty probe side
    with pytest.raises(ValueError):
        join(rows, [], [0], [0], LEFT)                                                            # width of the NULL tail unknown


def test_columns_may_repeat_and_a_list_may_be_empty():
    probe, build = [[1, "p"]], [[1, "b"]]
    assert join(probe, build, [0], [0], INNER, [1, 1, 0], []) == [["p", "p", 1]]
    assert join(probe, build, [0], [0], INNER, [], [1, 0, 1]) == [["b", 1, "b"]]
    with pytest.raises(ValueError):
        HashJoinOperator(Rows(probe), Rows(build), [0], [0], SEMI, [0], [1])
    with pytest.raises(ValueError):
        HashJoinOperator(Rows(probe), Rows(build), [], [], INNER)


def test_argument_checks_that_need_no_device(native_lib):
    lib = native_lib
    ctx = E.Context(device=None)
    try:
        schema_only = E.DeviceBatch.describe(ctx, [Column(DataType.INT64, np.arange(4, dtype=np.int64))])
        keys = (C.c_int32 * 1)(0)

        def build(inp):
            out = C.c_void_p(0xdead)
            st = lib.qe_join_build(ctx.handle, C.byref(inp) if inp is not None else None, keys, 1, C.byref(out))
            assert out.value is None
            return st

        assert build(N.JoinInput(None, schema_only.handle)) == INVALID_ARG
        assert b"schema-only" in lib.qe_last_error(ctx.handle)
        assert build(N.JoinInput(None, None)) == INVALID_ARG                                       # neither member
        assert build(N.JoinInput(schema_only.handle, schema_only.handle)) == INVALID_ARG           # both (checked before either is read)
        assert build(None) == INVALID_ARG
        assert lib.qe_join_build(ctx.handle, C.byref(N.JoinInput(None, schema_only.handle)), keys, 1, None) == INVALID_ARG
        assert lib.qe_join_table_rows(None) == -1
        stats = (C.c_int64 * 4)(*[7] * 4)
        assert lib.qe_ctx_last_join_stats(ctx.handle, stats) == 0 and list(stats) == [0, 0, 0, 0]
        assert lib.qe_batch_from_result(ctx.handle, None, C.byref(C.c_void_p())) == INVALID_ARG
        schema_only.free()
    finally:
        ctx.close()
