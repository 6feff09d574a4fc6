"""qe_result_asof_join on the device: for every left row the nearest earlier or later right row of its by partition.

The expectation is tests/asof_reference.py (numpy; proved equal to the host branch of ``AsofJoinOperator`` in
tests/test_asof_cpu.py).  Every output column is compared in full -- type, nullability, dictionary, validity, values by bits
(any NaN for any NaN), zero under the NULL of an unmatched LEFT row -- with no tolerance; counts and last_asof_stats are
checked too.  Where a case has an answer that can be written down without the reference (ties, partition edges, the sweep
boundary) it is asserted as well.  Sizes are those where the code changes path: word (64) and tile (2048) edges of the
bitmaps, a second side that lands at an unaligned bit offset, and more rows than one sweep of the kernels
(native.ASOF_BLOCKS blocks of 256 lanes).

Not tested: left rows + right rows >= 2^32 - 1 (QE_ERR_UNSUPPORTED; the inputs alone would be tens of GB); QE_ERR_OOM;
QE_ERR_HIP on a planning-only context (it cannot hold a result); a STRING by column without a dictionary, which cannot be
built through the ABI.  The errors decided from the scalar arguments alone are in tests/test_asof_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from queryengine_amd import Column, ColumnExpression, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N

from asof_reference import asof_reference
from window_reference import T, assert_window_output

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
BACK, FWD = N.ASOF_BACKWARD, N.ASOF_FORWARD
INNER, LEFT = N.JOIN_INNER, N.JOIN_LEFT
FORMS = [(d, s, j) for d in (BACK, FWD) for s in (False, True) for j in (INNER, LEFT)]
INVALID_ARG = 1
NAN, INF = float("nan"), float("inf")
STRINGS = ["b", "a", "", "B", "～", "\U0001F600", "aa", "Zü", "zz", "a "]     # not in sorted order
SEAM_LENGTHS = [2049, 1, 2048, 2, 65, 64, 63]
SEAM_DICT = [f"s{(7 * i) % 40:02d}" for i in range(40)]                       # 40 distinct strings, not in sorted order
SWEEP = N.ASOF_BLOCKS * 256         # sorted positions of one sweep of asof_eligible / asof_pick


def build(ctx, cols):
    """filter_project over an identity projection: a result that holds exactly `cols`."""
    batch = E.DeviceBatch.from_columns(ctx, cols)
    projs = [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)]
    return batch, E.filter_project(ctx, batch, None, projs)


def nullable_of(res):
    return [bool(res.view(c).nullable) for c in range(res.ncols)]


def column_bytes(result):
    return [(c.data.tobytes(), None if c.valid is None else c.valid.tobytes()) for c in result.to_columns()]


class Pair:
    """Two results on the device and the columns they were made of."""

    def __init__(self, ctx, lcols, rcols):
        self.ctx, self.lcols, self.rcols = ctx, lcols, rcols
        self.lbatch, self.lres = build(ctx, lcols)
        self.same = rcols is lcols
        self.rbatch, self.rres = (None, self.lres) if self.same else build(ctx, rcols)

    def check(self, left_by, right_by, left_on, right_on, form, left_out, right_out, what=""):
        """One qe_result_asof_join against the reference; returns (expected columns, expected stats)."""
        direction, strict, join_type = form
        what = f"{what}: {'FORWARD' if direction else 'BACKWARD'}{' strict' if strict else ''} {'LEFT' if join_type == LEFT else 'INNER'}"
        want, stats = asof_reference(self.lcols, self.rcols, nullable_of(self.lres), nullable_of(self.rres), left_by, right_by, left_on,
                                     right_on, direction, strict, join_type, left_out, right_out)
        out = self.ctx.asof_join(self.lres, self.rres, left_by, right_by, left_on, right_on, direction, strict, join_type, left_out, right_out)
        try:
            assert out.count == len(want[0].data), (what, out.count, len(want[0].data))
            assert self.ctx.last_asof_stats() == stats, (what, self.ctx.last_asof_stats(), stats)
            assert_window_output(out, want, what)
        finally:
            out.free()
        return want, stats

    def free(self):
        for r in (self.lres, self.lbatch) + (() if self.same else (self.rres, self.rbatch)):
            r.free()


def by_column(t, ids, k=0, dictionary=STRINGS):
    """A by column that is a function of the partition id: INT64 and DOUBLE one-to-one, the others folded."""
    v = ids + 3 * k
    if t == I64:
        return Column(I64, (ids * 3 - 50).astype(np.int64))
    if t == D:
        return Column(D, ids / 4.0 - 3.0)
    if t == I32:
        return Column(I32, (v % 7 - 3).astype(np.int32))
    if t == B:
        return Column(B, v % 3 == 0)
    return Column(S, (v % len(dictionary)).astype(np.int32), None, dictionary)


def with_nulls(col, rng, share=0.1):
    n = len(col)
    valid = rng.random(n) >= share
    if n > 1:
        valid[:2] = [True, False]       # never all ones: the bitmap stays
    noise = rng.integers(0, 2, n)
    data = np.where(valid, col.data, (noise % max(1, len(col.dictionary or [0, 1]))).astype(col.data.dtype))   # the value under a NULL is noise
    return Column(col.type, data, valid, col.dictionary)


def on_column(t, rng, n, span=12, nulls=0.1):
    """Few distinct values, so that equal `on` values meet inside a partition and across the sides."""
    v = rng.integers(-span, span, n)
    col = Column(t, v / 2.0 if t == D else v.astype(np.int64 if t == I64 else np.int32))
    return with_nulls(col, rng, nulls) if nulls else col


def payload(rng, n):
    """INT64 row id, nullable STRING."""
    tags = ["t0", "", "täg", "t3"]
    return [Column(I64, np.arange(n, dtype=np.int64)), Column(S, rng.integers(0, 4, n).astype(np.int32), (rng.random(n) > 0.2) if n else None, tags)]


def seam_ids(n, shift, rng):
    """n partition ids whose runs, in sorted order, have the seam lengths (the last run cut): they straddle word and 2048-row
    edges.  Shuffled, so that a cut anywhere deals every partition to both sides."""
    lengths = []
    while sum(lengths) < n:
        lengths.append(SEAM_LENGTHS[(len(lengths) + shift) % len(SEAM_LENGTHS)])
    ids = np.repeat(np.arange(len(lengths)), lengths)[:n]
    return ids[rng.permutation(n)].astype(np.int64)


# ---- 1. word and tile seams ------------------------------------------------------------------------------------------------------
SEAM_KEYS = [([I64], D), ([D, B], I64), ([S], I32), ([I32, I64], D)]


@pytest.mark.parametrize("aligned", [True, False], ids=["n-multiple-of-64", "n-ragged"])
@pytest.mark.parametrize("case, nl", list(enumerate([63, 64, 65, 3 * T + 37])))
def test_word_and_tile_seams(gpu_ctx, case, nl, aligned):
    rng = np.random.default_rng(700 + 2 * case + aligned)
    nr = 2 * T + (-nl) % 64 + (0 if aligned else 5)
    assert ((nl + nr) % 64 == 0) == aligned
    by_types, on_type = SEAM_KEYS[case]
    ids = seam_ids(nl + nr, case, rng)
    nby = len(by_types)

    assert ids.max() < len(SEAM_DICT)

    def side(part):           # an INT64, DOUBLE or STRING by column is one-to-one in the partition id: the runs stay as they are
        return [by_column(t, part, k, SEAM_DICT) for k, t in enumerate(by_types)] + [on_column(on_type, rng, len(part))] + payload(rng, len(part))
    pair = Pair(gpu_ctx, side(ids[:nl]), side(ids[nl:]))
    try:
        matched = {}
        for form in FORMS:
            _, stats = pair.check(list(range(nby)), list(range(nby)), nby, nby, form, [nby + 1, nby], [nby + 1, nby + 2, nby], f"seams nl {nl} nr {nr}")
            matched[form] = stats["matched"]
            assert stats["partitions"] >= 3
        assert all(0 < m < nl or nl < 70 for m in matched.values()) and matched[(BACK, True, LEFT)] <= matched[(BACK, False, LEFT)]
    finally:
        pair.free()


# ---- 2. partition edges: the match never leaks across a partition ---------------------------------------------------------------------
def test_partition_edges(gpu_ctx):
    """By partitions 0 .. 5 in sorted order; `on` is the position inside the partition.
       0: right rows only            1: left rows only (its neighbours hold only right rows)       2: right rows only
       3: left rows stand before every right row (backward: nothing) -- the eligible right row is the partition's LAST position
       4: left rows stand after every right row (forward: nothing) -- the eligible right row is the partition's FIRST position
       5: a left row between two right rows"""
    lby = np.array([1, 1, 1, 3, 3, 4, 4, 5], dtype=np.int32)
    lon = np.array([0, 5, 9, 0, 1, 7, 8, 5], dtype=np.int32)
    rby = np.array([0, 0, 2, 2, 3, 4, 5, 5], dtype=np.int32)
    ron = np.array([8, 9, 0, 1, 2, 6, 4, 6], dtype=np.int32)
    rng = np.random.default_rng(710)
    lp, rp = rng.permutation(len(lby)), rng.permutation(len(rby))
    lcols = [Column(I32, lby[lp]), Column(I32, lon[lp]), Column(I64, np.arange(8, dtype=np.int64))]
    rcols = [Column(I32, rby[rp]), Column(I32, ron[rp]), Column(I64, np.arange(8, dtype=np.int64))]
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 1, form, [0, 1], [0, 1, 2], "edges")
            assert stats["partitions"] == 6
            if form[2] == LEFT:
                found = {(int(b), int(o)): (int(want[3].data[i]) if want[3].valid[i] else None) for i, (b, o) in enumerate(zip(lcols[0].data, lcols[1].data))}
                assert all(found[(1, o)] is None for o in (0, 5, 9))                              # never the neighbours' rows
                assert [found[(3, 0)], found[(3, 1)]] == ([None, None] if form[0] == BACK else [2, 2])
                assert [found[(4, 7)], found[(4, 8)]] == ([6, 6] if form[0] == BACK else [None, None])
                assert found[(5, 5)] == (4 if form[0] == BACK else 6)
                assert all(want[2].data[i] == want[0].data[i] for i in range(8) if want[2].valid[i])   # the match has the left row's by value
    finally:
        pair.free()


# ---- 3. ties and strictness ------------------------------------------------------------------------------------------------------
def test_ties_and_strictness(gpu_ctx):
    """100 right rows and 70 left rows share on = 5 in one partition (both runs pass a word edge); right rows with on 3 and 8
    stand around them.  Not strict: the last (backward) / first (forward) of the hundred by right row index; strict: past them."""
    rng = np.random.default_rng(720)
    ron = np.concatenate([np.full(100, 5), np.full(3, 3), np.full(4, 8)]).astype(np.int64)
    rp = rng.permutation(len(ron))
    ron = ron[rp]
    lon = np.concatenate([np.full(70, 5), [4, 9, 2]]).astype(np.int64)[rng.permutation(73)]
    for nby in (0, 1):
        by = [Column(B, np.ones(len(lon), dtype=bool))] * nby, [Column(B, np.ones(len(ron), dtype=bool))] * nby
        pair = Pair(gpu_ctx, by[0] + [Column(I64, lon)], by[1] + [Column(I64, ron), Column(I64, np.arange(len(ron), dtype=np.int64))])
        rid = lambda v: np.nonzero(ron == v)[0]      # noqa: E731
        expect = {(BACK, False): {5: rid(5).max(), 4: rid(3).max(), 9: rid(8).max(), 2: None},
                  (BACK, True): {5: rid(3).max(), 4: rid(3).max(), 9: rid(8).max(), 2: None},
                  (FWD, False): {5: rid(5).min(), 4: rid(5).min(), 9: None, 2: rid(3).min()},
                  (FWD, True): {5: rid(8).min(), 4: rid(5).min(), 9: None, 2: rid(3).min()}}
        try:
            for form in FORMS:
                want, _ = pair.check(list(range(nby)), list(range(nby)), nby, nby, form, [nby], [nby + 1], f"ties nby {nby}")
                for v, r in zip(want[0].data, np.where(want[1].valid, want[1].data, -1)):          # every left row with one `on`: one match
                    assert (None if r < 0 else r) == expect[form[:2]][int(v)], (form, v, r)
        finally:
            pair.free()


# ---- 4. special values of `on` ---------------------------------------------------------------------------------------------------
ON_SPECIALS = {D: [NAN, -0.0, 0.0, INF, -INF, 1.5, -2.25, 5e-324],
               I64: [2 ** 53, 2 ** 53 + 1, 2 ** 53 - 1, -(2 ** 63), 2 ** 63 - 1, -(2 ** 53), -(2 ** 53) - 1, 0],
               I32: [-(2 ** 31), 2 ** 31 - 1, -1, 0, 1, -7]}


@pytest.mark.parametrize("on_type", [D, I64, I32], ids=["DOUBLE", "INT64", "INT32"])
def test_special_values_of_on(gpu_ctx, on_type):
    rng = np.random.default_rng(730 + int(on_type))
    nl, nr = 333, 290
    pool = np.array(ON_SPECIALS[on_type], dtype={D: np.float64, I64: np.int64, I32: np.int32}[on_type])
    if on_type == I64:
        assert len(set(pool.astype(np.float64))) < len(pool)                                 # pairs equal as doubles, different as integers
    lcols = [Column(I32, rng.integers(0, 3, nl).astype(np.int32)), Column(on_type, pool[rng.integers(0, len(pool), nl)])] + payload(rng, nl)
    rcols = [Column(I32, rng.integers(0, 3, nr).astype(np.int32)), Column(on_type, pool[rng.integers(0, len(pool), nr)])] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 1, form, [1, 2], [1, 2], f"special {on_type.name}")
            assert 0 < stats["matched"] <= nl and (stats["matched"] < nl or not form[1])      # strict: the extreme value finds nothing
    finally:
        pair.free()


# ---- 5. NULLs ----------------------------------------------------------------------------------------------------------------------
def test_nulls_match_nothing_and_hide_nothing(gpu_ctx):
    rng = np.random.default_rng(740)
    nl, nr = 3 * 64 + 7, 2 * 64 + 50
    lcols = [with_nulls(Column(I32, rng.integers(0, 4, nl).astype(np.int32)), rng, 0.2), on_column(I32, rng, nl, 6, 0.25)] + payload(rng, nl)
    rcols = [with_nulls(Column(I32, rng.integers(0, 4, nr).astype(np.int32)), rng, 0.2), on_column(I32, rng, nr, 6, 0.25)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 1, form, [0, 1, 2], [0, 1, 2], "nulls")
            assert stats["partitions"] == 5                                                     # NULL is one by value for the sort
            if form[2] == LEFT:
                no_key = ~(want[0].valid & want[1].valid)
                assert no_key.sum() > 40 and not want[5].valid[no_key].any()                   # a NULL by or on: no match, both directions
                assert want[3].valid[want[5].valid].all() and want[4].valid[want[5].valid].all()   # a match has a whole key
                assert want[5].valid.sum() == stats["matched"] > 40
    finally:
        pair.free()
    # a NULL `on` on the right is not picked and does not hide the valid row before it; NULL on the left: nothing, also forward
    rcols = [Column(I32, np.array([1, 2, 3], dtype=np.int32), np.array([True, False, True])), Column(I64, np.arange(3, dtype=np.int64))]
    lcols = [Column(I32, np.array([2, 0, 5], dtype=np.int32), np.array([True, False, True]))]
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        want, _ = pair.check([], [], 0, 0, (BACK, False, LEFT), [0], [1], "null on")
        assert np.where(want[1].valid, want[1].data, -1).tolist() == [0, -1, 2]
        want, _ = pair.check([], [], 0, 0, (FWD, False, LEFT), [0], [1], "null on")
        assert np.where(want[1].valid, want[1].data, -1).tolist() == [2, -1, -1]
    finally:
        pair.free()


# ---- 6. by keys of every type --------------------------------------------------------------------------------------------------------
BY_SETS = {0: [], 1: [S], 4: [B, S, I32, D], 7: [I64, B, S, D, I32, S, B]}


@pytest.mark.parametrize("nby", list(BY_SETS))
def test_by_columns_of_every_type(gpu_ctx, nby):
    rng = np.random.default_rng(750 + nby)
    nl, nr = 2 * T + 19, T + 45
    types = BY_SETS[nby]

    def side(n):
        ids = rng.integers(0, 40, n)
        by = [with_nulls(by_column(t, ids, k), rng, 0.05) for k, t in enumerate(types)]
        return by + [on_column(D, rng, n, 30)] + payload(rng, n)
    pair = Pair(gpu_ctx, side(nl), side(nr))
    try:
        for form in FORMS:
            _, stats = pair.check(list(range(nby)), list(range(nby)), nby, nby, form, [nby + 1], [nby + 1, nby + 2], f"nby {nby}")
            assert stats["matched"] > nl // 4 and (stats["partitions"] == 1) == (nby == 0)
    finally:
        pair.free()


LEFT_DICT = ["m", "b", "zz", "a"]
DICTS = {"same-object": (LEFT_DICT, LEFT_DICT), "reordered": (LEFT_DICT, LEFT_DICT[::-1]), "right-lacks-a-left-string": (LEFT_DICT, ["a", "q", "zz"]),
         "twice-listed": (["a", "b", "a"], ["b", "x", "b", "y", "a", "x"])}


@pytest.mark.parametrize("mode", list(DICTS))
def test_string_by_columns_compare_by_string(gpu_ctx, mode):
    rng = np.random.default_rng(760 + list(DICTS).index(mode))
    ld, rd = DICTS[mode]
    nl, nr = 200, 263
    lcols = [Column(S, rng.integers(0, len(ld), nl).astype(np.int32), rng.random(nl) > 0.1, ld), on_column(I32, rng, nl)] + payload(rng, nl)
    rcols = [Column(S, rng.integers(0, len(rd), nr).astype(np.int32), rng.random(nr) > 0.1, rd), on_column(I32, rng, nr)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 1, form, [0, 2], [0, 2], mode)
            assert want[0].dictionary == list(ld) and want[2].dictionary == list(rd)            # each column its source's dictionary
            assert stats["partitions"] == len(set(ld) | set(rd)) + 1 and stats["matched"] > 0
            ok = want[2].valid
            assert [ld[c] for c in want[0].data[ok]] == [rd[c] for c in want[2].data[ok]]       # the same string under whatever code
    finally:
        pair.free()


def test_double_by_columns_nan_and_signed_zero(gpu_ctx):
    rng = np.random.default_rng(770)
    nl, nr = 150, 170
    nans = np.array([0x7ff8000000000000, 0x7ff8000000000001, 0xfff8000000000000], dtype=np.uint64).view(np.float64)
    pool = np.concatenate([nans, [-0.0, 0.0, INF]])
    lcols = [Column(D, pool[rng.integers(0, 6, nl)]), on_column(I64, rng, nl)] + payload(rng, nl)
    rcols = [Column(D, pool[rng.integers(0, 6, nr)]), on_column(I64, rng, nr)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 1, form, [0], [0, 2], "double by")
            assert stats["partitions"] == 4                                                     # every NaN one value, -0.0 is not 0.0
            ok = want[1].valid
            assert np.array_equal(np.isnan(want[0].data[ok]), np.isnan(want[1].data[ok]))
            assert np.array_equal(np.signbit(want[0].data[ok & ~np.isnan(want[0].data)]), np.signbit(want[1].data[ok & ~np.isnan(want[0].data)]))
    finally:
        pair.free()


# ---- 7. more than one sweep of the kernels ----------------------------------------------------------------------------------------------
def test_one_partition_past_one_sweep(gpu_ctx):
    """No by column, n > SWEEP distinct `on` values: the left rows hold the odd ones, the right rows the even ones, so the row
    at sorted position j has on = j and the answer is known without the reference: on - 1 backward, on + 1 forward."""
    rng = np.random.default_rng(780)
    n = SWEEP + 2 * 64 + 78
    assert n > SWEEP and n % 2 == 0 and n % 64
    lon, ron = np.arange(1, n, 2, dtype=np.int64), np.arange(0, n, 2, dtype=np.int64)
    lon, ron = lon[rng.permutation(len(lon))], ron[rng.permutation(len(ron))]
    pair = Pair(gpu_ctx, [Column(I64, lon)], [Column(I64, ron), Column(I64, np.arange(len(ron), dtype=np.int64))])
    try:
        for form in ((BACK, False, LEFT), (FWD, True, INNER), (FWD, False, LEFT), (BACK, True, INNER)):
            want, stats = pair.check([], [], 0, 0, form, [0], [0, 1], "one partition past one sweep")
            assert stats == {"left_rows": n // 2, "right_rows": n // 2, "matched": n // 2 - (form[0] == FWD), "partitions": 1}
            step = 1 if form[0] == FWD else -1
            out = gpu_ctx.asof_join(pair.lres, pair.rres, [], [], 0, 0, *form, [0], [0, 1])
            mine, theirs, rid = out.column_to_host(0).data, out.column_to_host(1), out.column_to_host(2).data
            out.free()
            ok = theirs.valid if theirs.valid is not None else np.ones(len(mine), dtype=bool)
            assert np.array_equal(theirs.data[ok], mine[ok] + step) and np.array_equal(ron[rid[ok]], mine[ok] + step)
            at_seam = np.isin(mine, np.arange(SWEEP - 7, SWEEP + 8))                            # the left rows at the sweep boundary
            assert at_seam.sum() >= 7 and ok[at_seam].all()
            assert (~ok).sum() == (1 if form == (FWD, False, LEFT) else 0)                     # the last left row has no later right row
    finally:
        pair.free()


def test_many_partitions_past_one_sweep(gpu_ctx):
    rng = np.random.default_rng(790)
    nl, nr = SWEEP // 2 + 4001, SWEEP // 2 + 77
    lcols = [Column(I32, rng.integers(0, 3000, nl).astype(np.int32)), on_column(D, rng, nl, 50, 0.02), Column(I64, np.arange(nl, dtype=np.int64))]
    rcols = [Column(I32, rng.integers(0, 3000, nr).astype(np.int32)), on_column(D, rng, nr, 50, 0.02), Column(I64, np.arange(nr, dtype=np.int64))]
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in ((BACK, False, INNER), (FWD, True, LEFT)):
            _, stats = pair.check([0], [0], 1, 1, form, [2, 1], [2, 1], "many partitions past one sweep")
            assert stats["partitions"] == 3000 and nl // 2 < stats["matched"] < nl
    finally:
        pair.free()


# ---- 8. degenerate inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", ["left", "right", "both"])
def test_empty_sides(gpu_ctx, empty):
    rng = np.random.default_rng(800)
    n = 130
    full = [by_column(S, rng.integers(0, 5, n)), on_column(D, rng, n)] + payload(rng, n)
    none = [Column(c.type, c.data[:0], None, c.dictionary) for c in full]
    lcols, rcols = (none if empty in ("left", "both") else full), (none if empty in ("right", "both") else list(full))
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 1, form, [0, 1, 3], [2, 3, 0], f"{empty} empty")
            assert len(want) == 6 and stats["matched"] == 0
            assert len(want[0].data) == (n if empty == "right" and form[2] == LEFT else 0)
            assert (stats["partitions"] == 0) == (empty == "both")
            assert want[5].dictionary == STRINGS and [w.nullable for w in want[3:]] == ([True] * 3 if form[2] == LEFT else [False, bool(empty == "left"), False])
    finally:
        pair.free()


def test_self_join_lists_and_nullability(gpu_ctx):
    rng = np.random.default_rng(810)
    n = 2 * T + 3
    cols = [by_column(I32, rng.integers(0, 30, n)), on_column(I64, rng, n, 40, 0.05)] + payload(rng, n)
    pair = Pair(gpu_ctx, cols, cols)                  # the same handle on both sides
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 1, form, [2, 1], [2, 1], "self")
            if form == (BACK, False, LEFT):           # not strict: a row finds itself or a later row with its `on`
                ok = want[1].valid
                assert 0 < ok.sum() < n and want[2].valid[ok].all() and (want[2].data[ok] >= want[0].data[ok]).all() and np.array_equal(want[3].data[ok], want[1].data[ok])
            if form == (BACK, True, LEFT):            # strict: an earlier `on`
                ok = want[3].valid
                assert (want[3].data[ok] < want[1].data[ok]).all() and 0 < ok.sum() < n
        for form in ((BACK, False, LEFT), (FWD, True, INNER)):
            pair.check([0], [0], 1, 1, form, [2, 2, 3, 2], [3, 3], "a column listed twice")
            pair.check([0], [0], 1, 1, form, [], [2, 3], "no left column")
            pair.check([0], [0], 1, 1, form, [3, 2], [], "no right column")
            pair.check([0, 0], [0, 0], 1, 1, form, [2], [2], "a by column listed twice")
        want, _ = pair.check([0], [0], 1, 1, (FWD, False, LEFT), [0, 2], [0, 2], "nullability")
        assert [w.nullable for w in want] == [False, False, True, True]                       # LEFT: every right column nullable
        want, _ = pair.check([0], [0], 1, 1, (FWD, False, INNER), [0, 2, 3], [0, 2, 3], "nullability")
        assert [w.nullable for w in want] == [False, False, True] * 2                         # INNER: the source's
    finally:
        pair.free()


# ---- 9. determinism and reuse ------------------------------------------------------------------------------------------------------
def determinism_columns():
    rng = np.random.default_rng(820)
    nl, nr = 3 * T + 5, 2 * T + 71
    lcols = [with_nulls(by_column(S, rng.integers(0, 9, nl)), rng), by_column(D, rng.integers(0, 5, nl)), on_column(D, rng, nl, 40)] + payload(rng, nl)
    rcols = [with_nulls(by_column(S, rng.integers(0, 9, nr), 0, STRINGS[::-1]), rng), by_column(D, rng.integers(0, 5, nr)), on_column(D, rng, nr, 40)] + payload(rng, nr)
    return lcols, rcols


def test_the_same_bytes_on_every_run_and_on_a_fresh_context(gpu_ctx):
    lcols, rcols = determinism_columns()

    def run(ctx):
        pair = Pair(ctx, lcols, rcols)
        data = []
        for direction, strict, join_type in FORMS:
            out = ctx.asof_join(pair.lres, pair.rres, [0, 1], [0, 1], 2, 2, direction, strict, join_type, [3, 4, 2], [3, 4, 2, 0])
            data.append(column_bytes(out))
            out.free()
        pair.free()
        return data

    first = run(gpu_ctx)
    assert run(gpu_ctx) == first
    other = E.Context(device=0)
    try:
        assert run(other) == first
    finally:
        other.close()


def test_the_output_is_an_ordinary_result(gpu_ctx):
    ctx = gpu_ctx
    lcols, rcols = determinism_columns()
    pair = Pair(ctx, lcols, rcols)
    want, _ = asof_reference(lcols, rcols, nullable_of(pair.lres), nullable_of(pair.rres), [0, 1], [0, 1], 2, 2, BACK, False, LEFT, [3, 2], [3, 2])
    out = ctx.asof_join(pair.lres, pair.rres, [0, 1], [0, 1], 2, 2, BACK, False, LEFT, [3, 2], [3, 2])
    pair.free()                                                                                 # the output owns its buffers
    assert_window_output(out, want, "after the inputs were freed")
    batch = out.as_batch()                                                                      # qe_batch_from_result: the next plan's input
    again = E.filter_project(ctx, batch, None, [ctx.compile(ColumnExpression(f"c{i}", i, w.type)) for i, w in enumerate(want)])
    assert_window_output(again, [type(w)(w.type, w.data, w.valid, w.nullable, w.dictionary) for w in want], "through qe_batch_from_result")
    by_rid = ctx.order_by_keys(out, [(2, True), (0, False)])                                    # matched row id descending, NULL last
    got = by_rid.column_to_host(2)
    nvalid = int(want[2].valid.sum())
    gv = got.valid if got.valid is not None else np.ones(len(got), dtype=bool)
    assert 0 < nvalid < out.count == by_rid.count and np.all(np.diff(got.data[:nvalid]) <= 0) and not gv[nvalid:].any() and gv[:nvalid].all()
    second = ctx.asof_join(out, out, [], [], 0, 0, FWD, True, INNER, [0], [0])                  # and into another ASOF join, with itself
    assert second.count == out.count - 1 and np.array_equal(second.column_to_host(1).data, second.column_to_host(0).data + 1)
    for r in (second, by_rid, again, batch, out):
        r.free()


def test_operator_on_gpu_sources_matches_its_host_branch(gpu_ctx):
    from queryengine_amd import ColumnarTable, Field, Schema
    from queryengine_amd.operators import AsofJoinOperator, GpuFilterProjectOperator, map as op_map
    from test_setop_cpu import Rows, assert_rows
    rng = np.random.default_rng(830)

    def table(n, dictionary):
        cols = [Column(S, rng.integers(0, len(dictionary), n).astype(np.int32), rng.random(n) > 0.2, dictionary),
                Column(D, np.array([NAN, -0.0, 0.0, 1.5, -INF])[rng.integers(0, 5, n)], rng.random(n) > 0.2), Column(I64, np.arange(n, dtype=np.int64))]
        return cols, ColumnarTable(Schema([Field("k", S), Field("t", D), Field("id", I64)]), cols)
    (lcols, ltable), (rcols, rtable) = table(150, ["a", "b", "c"]), table(170, ["c", "d", "a"])
    exprs = [ColumnExpression("k", 0, S), ColumnExpression("t", 1, D), ColumnExpression("id", 2, I64)]
    boxed = lambda cols, n: [[c.value(i) for c in cols] for i in range(n)]      # noqa: E731
    for direction, strict, join_type in FORMS:
        left = GpuFilterProjectOperator(gpu_ctx, ltable.getScanOperator(["k", "t", "id"]), None, exprs)
        right = GpuFilterProjectOperator(gpu_ctx, rtable.getScanOperator(["k", "t", "id"]), None, exprs)
        dev = op_map(AsofJoinOperator(left, right, [0], [0], 1, 1, direction, strict, join_type), list)
        host = op_map(AsofJoinOperator(Rows(boxed(lcols, 150)), Rows(boxed(rcols, 170)), [0], [0], 1, 1, direction, strict, join_type,
                                       right_out=[0, 1, 2]), list)
        assert_rows(dev, host, f"direction {direction} strict {strict} join {join_type}")


@pytest.mark.parametrize("nl, nr", [(1, 0), (0, 1), (1, 1), (40, 24), (40, 25), (1000, 25)], ids=lambda v: str(v))
def test_small_totals_against_the_host_operator(gpu_ctx, nl, nr):
    """nl + nr = 1, 2, 64, 65 (the word edge of the partition-start bitmap) and 1025 (past one 1024-row block of the radix
    histogram), by a nullable STRING column whose sides carry different dictionaries that share some strings."""
    from queryengine_amd.operators import AsofJoinOperator, map as op_map
    from test_setop_cpu import Rows, assert_rows
    rng = np.random.default_rng(835 + nl + nr)

    def side(n, dictionary):
        valid = rng.random(n) > 0.2 if n else None
        if n > 1:
            valid[:2] = [True, False]       # never all ones: the bitmap stays
        return [Column(S, rng.integers(0, len(dictionary), n).astype(np.int32), valid, dictionary), on_column(I64, rng, n, 6, 0.0),
                Column(I64, np.arange(n, dtype=np.int64))]
    lcols, rcols = side(nl, ["m", "b", "zz", "a"]), side(nr, ["a", "q", "zz", "c"])
    boxed = lambda cols, n: [[c.value(i) for c in cols] for i in range(n)]      # noqa: E731
    lrows, rrows = boxed(lcols, nl), boxed(rcols, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for direction, strict, join_type in FORMS:
            host = op_map(AsofJoinOperator(Rows(lrows), Rows(rrows), [0], [0], 1, 1, direction, strict, join_type, right_out=[0, 1, 2]), list)
            out = gpu_ctx.asof_join(pair.lres, pair.rres, [0], [0], 1, 1, direction, strict, join_type, [0, 1, 2], [0, 1, 2])
            try:
                assert_rows(boxed(out.to_columns(), out.count), host, f"nl {nl} nr {nr} direction {direction} strict {strict} join {join_type}")
                assert gpu_ctx.last_asof_stats() == {"left_rows": nl, "right_rows": nr, "matched": sum(1 for row in host if row[5] is not None),
                                                     "partitions": len({row[0] for row in lrows + rrows})}
            finally:
                out.free()
    finally:
        pair.free()


# ---- 10. the errors that need a result to look at -----------------------------------------------------------------------------------
def test_invalid_arguments(gpu_ctx):
    ctx = gpu_ctx
    lib = ctx._lib
    rng = np.random.default_rng(840)
    n = 50
    cols = [Column(I32, rng.integers(0, 5, n).astype(np.int32)), Column(D, rng.normal(0, 1, n)), Column(S, rng.integers(0, 3, n).astype(np.int32), None, STRINGS),
            Column(B, rng.random(n) > 0.5), Column(I64, np.arange(n, dtype=np.int64))]
    pair = Pair(ctx, cols, cols)
    res = pair.lres

    def call(left_by=(0,), right_by=(0,), left_on=1, right_on=1, direction=0, strict=0, join_type=LEFT, left_out=(4,), right_out=(4,), null=()):
        out = C.c_void_p(0xdead)
        arr = lambda v: (C.c_int32 * max(1, len(v)))(*v)     # noqa: E731
        st = lib.qe_result_asof_join(None if "ctx" in null else ctx.handle, None if "left" in null else res.handle, None if "right" in null else res.handle,
                                     arr(left_by), arr(right_by), len(left_by), left_on, right_on, direction, strict, join_type,
                                     arr(left_out), len(left_out), arr(right_out), len(right_out), None if "out" in null else C.byref(out))
        if "out" not in null:
            if st != N.OK:
                assert out.value is None, "*out must be NULL after an error"
            else:
                lib.qe_result_free(ctx.handle, out)
        return st

    try:
        assert call() == N.OK
        for null in ("ctx", "left", "right", "out"):
            assert call(null=(null,)) == INVALID_ARG, null
        for bad in (dict(left_by=(5,)), dict(right_by=(-1,)), dict(left_on=5), dict(right_on=-1), dict(left_out=(5,)), dict(right_out=(4, -1)),   # out of range
                    dict(left_by=(0,), right_by=(4,)), dict(left_by=(0, 2), right_by=(0, 3)),                   # paired by columns of different types
                    dict(left_on=2, right_on=2), dict(left_on=3, right_on=3),                                   # `on` STRING, BOOLEAN
                    dict(left_on=1, right_on=4), dict(left_on=0, right_on=4),                                   # `on` types differ
                    dict(left_by=tuple(range(5)) + (0, 1, 2), right_by=tuple(range(5)) + (0, 1, 2)),            # eight by columns
                    dict(direction=2), dict(strict=2), dict(join_type=N.JOIN_SEMI), dict(left_out=(), right_out=())):
            assert call(**bad) == INVALID_ARG, bad
        assert call(left_by=(), right_by=(), left_on=4, right_on=4) == N.OK and call(left_on=0, right_on=0) == N.OK
        assert call(left_by=tuple(range(5)) + (0, 2), right_by=tuple(range(5)) + (0, 2)) == N.OK               # seven by columns
        pair.check([0, 2, 3], [0, 2, 3], 1, 1, (BACK, False, LEFT), [4], [4], "after the errors")              # the context still works
    finally:
        pair.free()
