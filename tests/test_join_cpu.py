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


# ---- tests/join_reference.py against the host branch: the proof that the numpy reference may stand in for it ----------------
from join_reference import assert_join_output, expected_columns, expected_nullable, match_counts, reference_pairs  # noqa: E402
from test_gpu_order_by_keys import DOUBLES, INT64S, make_key                                                          # noqa: E402

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
JOIN_TYPES = [INNER, LEFT, SEMI, ANTI]
JOIN_NAMES = {INNER: "INNER", LEFT: "LEFT", SEMI: "SEMI", ANTI: "ANTI"}
TAGS = ["t0", "", "täg", "t3"]
KEY_TYPES = [(D,), (I64,), (I32,), (S,), (B,), (D, S), (I64, B), (I32, I64), (S, D), (B, I32), (B, I64, D, S), (I32, S, D, I64), (S, B, I32, D)]


def payload(rng, n):
    """(INT64 row id, nullable BOOLEAN, nullable STRING, INT32, DOUBLE with NaN and -0.0)."""
    dbl = np.where(rng.random(n) < 0.1, np.array([NAN, -0.0])[rng.integers(0, 2, n)], rng.integers(-50, 50, n).astype(np.float64))
    return [Column(I64, np.arange(n, dtype=np.int64)), Column(B, rng.random(n) > 0.3, (rng.random(n) > 0.2) if n else None),
            Column(S, rng.integers(0, len(TAGS), n).astype(np.int32), (rng.random(n) > 0.1) if n else None, TAGS),
            Column(I32, rng.integers(-9, 9, n).astype(np.int32)), Column(D, dbl)]


def few(c):
    """The special-value pools cut down to a few values per column, so that whole tuples of several columns meet."""
    if c.type == S:
        return Column(S, c.data % 3, c.valid, c.dictionary)
    if c.type == D:
        return Column(D, np.where(np.isin(c.data, DOUBLES[:2]) | np.isnan(c.data), c.data, 1.5), c.valid)     # 0.0, -0.0, NaN, 1.5
    if c.type == I64:
        return Column(I64, np.where(np.isin(c.data, INT64S[3:5]), c.data, 0), c.valid)                          # max, min, 0
    if c.type == I32:
        return Column(I32, c.data % 4, c.valid)
    return c


def boxed(cols):
    lists = [c.to_list() for c in cols]
    return [[l[i] for l in lists] for i in range(len(cols[0]))]


def check_against_host(pcols, bcols, pk, bk, what=""):
    """reference_pairs and expected_columns against the host branch, for all four join types.  Every side ends in the
    payload whose first column is the row id.  -> {join type: number of output rows}"""
    prid, brid = len(pcols) - 5, len(bcols) - 5
    probe_out, build_all = list(range(prid, len(pcols))) + [pk[0]], list(range(brid, len(bcols))) + [bk[0]]
    prows, brows = boxed(pcols), boxed(bcols)
    sizes = {}
    for jt in JOIN_TYPES:
        build_out = build_all if jt in (INNER, LEFT) else []
        host = join(prows, brows, pk, bk, jt, probe_out, build_out)
        prow, brow = reference_pairs(pcols, bcols, pk, bk, jt)
        assert prow.dtype == np.int64 and brow.dtype == np.int64
        name = f"{what} {JOIN_NAMES[jt]}"
        assert [r[0] for r in host] == prow.tolist(), name                           # the probe row ids, pair for pair
        if jt in (INNER, LEFT):
            assert [r[len(probe_out)] for r in host] == [None if b < 0 else b for b in brow.tolist()], name
            assert (brow >= 0).all() or jt == LEFT
        else:
            assert len(brow) == 0
        want = expected_columns(pcols, bcols, prow, brow, probe_out, build_out, jt)
        assert same(boxed(want) if len(prow) else [], host), name                    # every value of every output column
        for c, w in zip(build_out, want[len(probe_out):]):                           # the zeroed value under "none"
            assert not w.data[brow < 0].any()
        assert_join_output(want, want, brow if jt in (INNER, LEFT) else None, len(probe_out), name)
        sizes[jt] = len(prow)
    cnt = match_counts(pcols, bcols, pk, bk)
    assert sizes[INNER] == int(cnt.sum()) and sizes[SEMI] == int((cnt > 0).sum()) and sizes[SEMI] + sizes[ANTI] == len(pcols[0])
    assert sizes[LEFT] == sizes[INNER] + sizes[ANTI]
    return sizes


@pytest.mark.parametrize("types", KEY_TYPES, ids=lambda ts: "-".join(t.name for t in ts))
def test_reference_pairs_equal_the_host_branch(types):
    matched = 0
    big = {1: (400, 200), 2: (600, 300), 4: (1500, 700)}[len(types)]      # (fewer key columns: fewer distinct keys, many more pairs to box)
    for np_, nb in ((0, 5), (5, 0), (1, 1), (63, 64), (257, 129), big):
        rng = np.random.default_rng([50, len(types), int(types[0]), np_])
        cut = few if len(types) > 1 else (lambda c: c)
        pcols = [cut(make_key(t, rng, np_, coarse=True)) for t in types] + payload(rng, np_)
        bcols = [cut(make_key(t, rng, nb, coarse=True)) for t in types] + payload(rng, nb)
        keys = list(range(len(types)))
        matched += check_against_host(pcols, bcols, keys, keys, f"{np_}x{nb}")[INNER]
    assert matched > 2 * big[0]                                                      # duplicate keys on both sides


def test_reference_pairs_with_fine_keys_and_key_columns_in_another_order():
    rng = np.random.default_rng(51)
    np_, nb = 1200, 800
    types = (I64, D, I32)
    pcols = [make_key(t, rng, np_, coarse=False, null_share=0.03) for t in types] + payload(rng, np_)
    bcols = [make_key(t, rng, nb, coarse=False, null_share=0.03) for t in types] + payload(rng, nb)
    for k in range(3):                                                               # one key column at a time: fine values meet
        sizes = check_against_host(pcols, bcols, [k], [k], f"key {k}")
        assert (0 if types[k] == I32 else 1) <= sizes[SEMI] < np_                    # (INT32 over its whole range meets nothing)
    pc = [few(c) for c in pcols[:3]] + pcols[3:]
    bc = [few(c) for c in bcols[:3]] + bcols[3:]
    swapped = [bc[2], bc[0], bc[1]] + bc[3:]                                          # key columns pair by position
    a = reference_pairs(pc, bc, [0, 1, 2], [0, 1, 2], INNER)
    b = reference_pairs(pc, swapped, [0, 1, 2], [1, 2, 0], INNER)
    assert len(a[0]) > 0 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    check_against_host(pc, swapped, [0, 1, 2], [1, 2, 0], "swapped")


def test_reference_pairs_across_two_dictionaries_with_a_duplicate_entry():
    rng = np.random.default_rng(31)
    pdict = ["x", "b", "a", "q", "～", "aa", "\U0001F600"]                     # "x", "q" only here
    bdict = ["aa", "a", "zz", "b", "\U0001F600", "～", "a", "Zü"]               # "zz", "Zü" only here; "a" listed twice
    np_, nb = 1500, 333
    pcols = [Column(S, rng.integers(0, len(pdict), np_).astype(np.int32), rng.random(np_) > 0.05, pdict)] + payload(rng, np_)
    bcols = [Column(S, rng.integers(0, len(bdict), nb).astype(np.int32), rng.random(nb) > 0.05, bdict)] + payload(rng, nb)
    check_against_host(pcols, bcols, [0], [0])
    prow, brow = reference_pairs(pcols, bcols, [0], [0], INNER)
    a = pcols[0].data[prow] == pdict.index("a")
    assert a.any() and set(bcols[0].data[brow[a]].tolist()) == {1, 6}               # both spellings of "a" on the build side
    anti, _ = reference_pairs(pcols, bcols, [0], [0], ANTI)
    assert {pcols[0].value(p) for p in anti.tolist()} >= {"x", "q", None}


def test_reference_pairs_with_a_side_of_all_null_keys_and_empty_sides():
    rng = np.random.default_rng(52)
    n = 300
    keyed = [Column(I32, rng.integers(0, 20, n).astype(np.int32))] + payload(rng, n)
    nulls = [Column(I32, rng.integers(0, 20, n).astype(np.int32), np.zeros(n, dtype=bool))] + payload(rng, n)
    empty = [Column(I32, np.zeros(0, dtype=np.int32))] + payload(rng, 0)
    for pcols, bcols, inner, anti in ((keyed, nulls, 0, n), (nulls, keyed, 0, n), (nulls, nulls, 0, n), (keyed, empty, 0, n),
                                      (empty, keyed, 0, 0), (empty, empty, 0, 0)):
        sizes = check_against_host(pcols, bcols, [0], [0])
        assert sizes == {INNER: inner, LEFT: inner + anti, SEMI: 0, ANTI: anti}
    two_p = [keyed[0], nulls[0]] + payload(rng, n)                                    # NULL in ONE of two key columns
    two_b = [keyed[0], keyed[0]] + payload(rng, n)
    assert check_against_host(two_p, two_b, [0, 1], [0, 1])[INNER] == 0
    assert check_against_host(two_b, two_b, [0, 1], [0, 1])[INNER] > n


def test_the_whole_column_checker_sees_one_wrong_bit():
    """assert_join_output is what the device tests trust: one wrong value, validity bit, NaN payload, zero sign or non-zero
    value under "none" in any column must fail it."""
    rng = np.random.default_rng(53)
    n = 400
    pcols = [Column(I32, rng.integers(0, 60, n).astype(np.int32))] + payload(rng, n)
    bcols = [Column(I32, rng.integers(0, 40, n).astype(np.int32))] + payload(rng, n)
    out_cols = [1, 2, 3, 4, 5]
    prow, brow = reference_pairs(pcols, bcols, [0], [0], LEFT)
    none = np.nonzero(brow < 0)[0]
    assert 0 < len(none) < len(brow)
    want = expected_columns(pcols, bcols, prow, brow, out_cols, out_cols, LEFT)
    assert expected_nullable([c.valid is not None for c in pcols], [c.valid is not None for c in bcols], out_cols, out_cols, LEFT) == \
        [False, True, True, False, False] + [True] * 5
    assert expected_nullable([False] * 6, [False, True, False, False, False, False], [1], [0, 1], INNER) == [False, False, True]

    def copy(cols):
        return [Column(c.type, c.data.copy(), None if c.valid is None else c.valid.copy(), c.dictionary) for c in cols]

    assert_join_output(copy(want), want, brow, 5)
    for k in range(10):
        valid_rows = np.nonzero(want[k].valid if want[k].valid is not None else np.ones(len(prow), dtype=bool))[0]
        for j in (valid_rows[0], valid_rows[len(valid_rows) // 2], valid_rows[-1]):
            bad = copy(want)
            if bad[k].type == D:
                bad[k].data.view(np.uint64)[j] ^= np.uint64(1)                        # the last bit of the mantissa (or of a NaN's payload)
            else:
                bad[k].data[j] = (not bad[k].data[j]) if bad[k].type == B else bad[k].data[j] + 1
            with pytest.raises(AssertionError):
                assert_join_output(bad, want, brow, 5)
            bad = copy(want)
            v = np.ones(len(prow), dtype=bool) if bad[k].valid is None else bad[k].valid
            v[j] = False
            bad[k] = Column(bad[k].type, bad[k].data, v, bad[k].dictionary)
            with pytest.raises(AssertionError):
                assert_join_output(bad, want, brow, 5)
        if k >= 5:                                                                    # a build column: a value under "none"
            bad = copy(want)
            bad[k].data[none[-1]] = 1
            with pytest.raises(AssertionError):
                assert_join_output(bad, want, brow, 5)
            assert_join_output(bad, want, None, 5)                                    # (seen only through brow: the row is invalid)
    dbl = want[4].data
    for value, other in ((-0.0, 0.0), (NAN, float(np.frombuffer(np.uint64(0xfff8000000000123).tobytes(), dtype=np.float64)[0]))):
        j = np.nonzero(np.isnan(dbl) if value != value else (dbl == 0.0) & np.signbit(dbl))[0][0]
        bad = copy(want)
        bad[4].data[j] = other
        with pytest.raises(AssertionError):
            assert_join_output(bad, want, brow, 5)
    bad = copy(want)
    bad[2] = Column(S, bad[2].data, bad[2].valid, TAGS[::-1])
    with pytest.raises(AssertionError):
        assert_join_output(bad, want, brow, 5)
    with pytest.raises(AssertionError):
        assert_join_output(copy(want)[:-1], want, brow, 5)
