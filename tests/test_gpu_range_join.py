"""qe_result_range_join on the device: for every left row all right rows of its by partition inside its interval.

The expectation is tests/range_join_reference.py (numpy; proved equal to the host branch of ``RangeJoinOperator`` in
tests/test_range_join_cpu.py).  Every output column is compared in full -- type, nullability, dictionary, validity, values by
bits (any NaN for any NaN), zero under the NULL of an unmatched LEFT row -- with no tolerance; counts and last_range_stats are
checked too.  Where a case has an answer that can be written down without the reference (the expansion's tiles, the skewed
row, ties, the hash join) it is asserted as well.  Sizes are those where the code changes path: word (64) and tile (2048)
edges of the bitmaps, 1024-element blocks of the scans and a second trip of their block sums, the tile of the expansion
(native.RANGE_EXPAND_TILE output rows), and more rows than one sweep of the kernels (native.RANGE_BLOCKS blocks of 256 lanes).

Not tested: outputs beyond 2^32 rows and left rows + right rows >= 2^32 - 1 (the buffers alone would be tens of GB);
QE_ERR_OOM; QE_ERR_HIP on a planning-only context (it cannot hold a result); a STRING by column without a dictionary, which
cannot be built through the ABI.  The errors decided from the scalar arguments alone are in tests/test_range_join_cpu.py."""
import ctypes as C
import random

import numpy as np
import pytest

from queryengine_amd import Column, ColumnExpression, DataType, Function, FunctionExpression, NumericLiteralExpression
from queryengine_amd import engine as E
from queryengine_amd import native as N

from range_join_reference import range_reference
from test_gpu_asof import (BY_SETS, DICTS, ON_SPECIALS, SEAM_DICT, STRINGS, build, by_column, column_bytes, nullable_of, payload, seam_ids,
                           with_nulls)
from window_reference import T, assert_window_output

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
INNER, LEFT, SEMI, ANTI = N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI
JOINS = [INNER, LEFT, SEMI, ANTI]
JOIN_NAMES = {INNER: "INNER", LEFT: "LEFT", SEMI: "SEMI", ANTI: "ANTI"}
STRICTS = [(False, False), (False, True), (True, False), (True, True)]
FORMS = [(ls, hs, j) for j in JOINS for ls, hs in STRICTS]
INVALID_ARG = 1
NAN, INF = float("nan"), float("inf")
NP = {D: np.float64, I64: np.int64, I32: np.int32}
TILE = N.RANGE_EXPAND_TILE
SWEEP = N.RANGE_BLOCKS * 256        # rows of one sweep of range_ordinals / range_counts


class Pair:
    """Two results on the device and the columns they were made of."""

    def __init__(self, ctx, lcols, rcols):
        self.ctx, self.lcols, self.rcols = ctx, lcols, rcols
        self.lbatch, self.lres = build(ctx, lcols)
        self.same = rcols is lcols
        self.rbatch, self.rres = (None, self.lres) if self.same else build(ctx, rcols)

    def check(self, left_by, right_by, lo, hi, on, form, left_out, right_out, what=""):
        """One qe_result_range_join against the reference; returns (expected columns, expected stats)."""
        lo_strict, hi_strict, join_type = form
        right_out = right_out if join_type in (INNER, LEFT) else []
        what = f"{what}: {'(' if lo_strict else '['}lo, hi{')' if hi_strict else ']'} {JOIN_NAMES[join_type]}"
        want, stats = range_reference(self.lcols, self.rcols, nullable_of(self.lres), nullable_of(self.rres), left_by, right_by, lo, hi, on,
                                      lo_strict, hi_strict, join_type, left_out, right_out)
        out = self.ctx.range_join(self.lres, self.rres, left_by, right_by, lo, hi, on, lo_strict, hi_strict, join_type, left_out, right_out)
        try:
            assert out.count == stats["output_rows"], (what, out.count, stats)
            assert self.ctx.last_range_stats() == stats, (what, self.ctx.last_range_stats(), stats)
            assert_window_output(out, want, what)
        finally:
            out.free()
        return want, stats

    def free(self):
        for r in (self.lres, self.lbatch) + (() if self.same else (self.rres, self.rbatch)):
            r.free()


def value_column(t, rng, n, span=12, nulls=0.1):
    """Few distinct values, so that equal values meet inside a partition and across the sides."""
    v = rng.integers(-span, span, n)
    col = Column(t, v / 2.0 if t == D else v.astype(NP[t]))
    return with_nulls(col, rng, nulls) if nulls else col


def bounds(t, rng, n, span=12, nulls=0.1, width=6):
    """(lo, hi) with hi - lo in [-2, width): some intervals are reversed, some a single value."""
    lo = rng.integers(-span, span, n)
    hi = lo + rng.integers(-2, width, n)
    cols = [Column(t, v / 2.0 if t == D else v.astype(NP[t])) for v in (lo, hi)]
    return [with_nulls(c, rng, nulls) for c in cols] if nulls else cols


# ---- 1. word and tile seams ------------------------------------------------------------------------------------------------------
SEAM_KEYS = [([I64], D), ([D, B], I64), ([S], I32), ([I32, I64], D)]


@pytest.mark.parametrize("aligned", [True, False], ids=["n-multiple-of-64", "n-ragged"])
@pytest.mark.parametrize("case, nl", list(enumerate([63, 64, 65, 3 * T + 37])))
def test_word_and_tile_seams(gpu_ctx, case, nl, aligned):
    rng = np.random.default_rng(900 + 2 * case + aligned)
    nr = 2 * T + (-nl) % 64 + (0 if aligned else 5)
    assert ((nl + nr) % 64 == 0) == aligned
    by_types, value_type = SEAM_KEYS[case]
    ids = seam_ids(nl + nr, case, rng)       # partitions in runs of 2049, 1, 2048, 2, 65, 64 and 63 rows
    nby = len(by_types)
    assert ids.max() < len(SEAM_DICT)
    by = lambda part: [by_column(t, part, k, SEAM_DICT) for k, t in enumerate(by_types)]      # noqa: E731
    lcols = by(ids[:nl]) + bounds(value_type, rng, nl) + payload(rng, nl)
    rcols = by(ids[nl:]) + [value_column(value_type, rng, nr)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        rows = {}
        for form in FORMS:
            _, stats = pair.check(list(range(nby)), list(range(nby)), nby, nby + 1, nby, form, [nby + 2, nby], [nby + 1, nby + 2, nby],
                                  f"seams nl {nl} nr {nr}")
            rows[form] = stats["output_rows"]
        for ls, hs in STRICTS:
            inner, left, semi, anti = (rows[(ls, hs, j)] for j in JOINS)
            assert semi + anti == nl and left == inner + anti and inner >= semi > 0 and anti > 0
        assert rows[(True, True, INNER)] < rows[(False, True, INNER)] < rows[(False, False, INNER)]
    finally:
        pair.free()


# ---- 2. the offset scan: its 1024-element blocks, and a second trip of the block sums ------------------------------------------------
@pytest.mark.parametrize("nl", [1023, 1024, 1025])
def test_scan_seams(gpu_ctx, nl):
    rng = np.random.default_rng(910 + nl)
    nr = 700
    lcols = [by_column(I32, rng.integers(0, 5, nl))] + bounds(I64, rng, nl, 20, 0.05, 9) + payload(rng, nl)
    rcols = [by_column(I32, rng.integers(0, 5, nr)), value_column(I64, rng, nr, 20, 0.05)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            _, stats = pair.check([0], [0], 1, 2, 1, form, [3, 1], [2, 1], f"scan nl {nl}")
            assert stats["output_rows"] > (nl if form[2] in (INNER, LEFT) else 100)
    finally:
        pair.free()


def test_scan_block_sums_take_a_second_trip(gpu_ctx):
    """2^20 + 65 left rows: 1025 block sums, one more than a trip of the carry scan.  Every left row asks for one value of
    the 1000 distinct ones on the right or for one that is not there, so the output is about as long as the left side."""
    rng = np.random.default_rng(915)
    nl, nr = (1 << 20) + 65, 1000
    v = rng.integers(0, 1200, nl).astype(np.int32)
    on = rng.permutation(nr).astype(np.int32)
    where = np.argsort(on)
    pair = Pair(gpu_ctx, [Column(I32, v), Column(I32, np.arange(nl, dtype=np.int32))], [Column(I32, on), Column(I32, np.arange(nr, dtype=np.int32))])
    try:
        hit = v < nr
        for form in ((False, False, INNER), (False, False, LEFT), (False, False, ANTI)):
            want, stats = pair.check([], [], 0, 0, 0, form, [1], [1], "2^20 + 65 left rows")
            assert stats["longest"] == 1 and stats["output_rows"] == {INNER: hit.sum(), LEFT: nl, ANTI: nl - hit.sum()}[form[2]]
            if form[2] == INNER:
                assert np.array_equal(want[0].data, np.nonzero(hit)[0]) and np.array_equal(want[1].data, where[v[hit]])
    finally:
        pair.free()


# ---- 3. the expansion's tiles ------------------------------------------------------------------------------------------------------
def pair_from_counts(ctx, counts, rng):
    """nby = 0, the right side holds the distinct values 0 .. nr - 1 shuffled; left row i asks for counts[i] consecutive values
    (0: a reversed interval).  Returns (pair, first value of every left row, right row of every value)."""
    counts = np.asarray(counts, dtype=np.int64)
    nr = int(counts.max()) + 11
    start = (np.arange(len(counts)) * 7) % (nr - counts + 1)
    lo = np.where(counts > 0, start, 5).astype(np.int32)
    hi = np.where(counts > 0, start + counts - 1, 4).astype(np.int32)
    on = rng.permutation(nr).astype(np.int32)
    pair = Pair(ctx, [Column(I32, lo), Column(I32, hi), Column(I32, np.arange(len(counts), dtype=np.int32))],
                [Column(I32, on), Column(I64, np.arange(nr, dtype=np.int64))])
    return pair, start, np.argsort(on)


EXPANSIONS = {
    "total T - 1": [3, 0, TILE - 1 - 3 - 5, 5],
    "total T": [3, 0, TILE - 3 - 5, 5],
    "total T + 1": [3, 0, TILE + 1 - 3 - 5, 5],
    "total 3 T + 5": [TILE, 5, 0, 0, 2 * TILE - 7, 7],
    "starts on a tile's last slot, spans more than two tiles": [TILE - 1, 2 * TILE + 7, 3],
    "ends on a tile's edge": [TILE - 5, 5, 9, TILE - 9, 1],
    "more than T rows without a match between two with": [4] + [0] * (TILE + 50) + [6],
    "every left row one match": [1] * (2 * TILE + 3),
}


@pytest.mark.parametrize("name", list(EXPANSIONS))
def test_expansion_seams(gpu_ctx, name):
    counts = np.asarray(EXPANSIONS[name], dtype=np.int64)
    pair, start, where = pair_from_counts(gpu_ctx, counts, np.random.default_rng(920 + len(name)))
    try:
        for join_type in (INNER, LEFT):
            want, stats = pair.check([], [], 0, 1, 0, (False, False, join_type), [2], [1, 0], name)
            emit = np.maximum(counts, 1) if join_type == LEFT else counts
            assert stats["output_rows"] == emit.sum() and stats["longest"] == counts.max()
            out = gpu_ctx.range_join(pair.lres, pair.rres, [], [], 0, 1, 0, False, False, join_type, [2], [1, 0])
            lrow, rrow, on = (out.column_to_host(c) for c in range(3))
            out.free()
            assert np.array_equal(lrow.data, np.repeat(np.arange(len(counts)), emit))               # the closed form
            found = np.repeat(counts > 0, emit)
            values = np.concatenate([np.arange(s, s + c) for s, c in zip(start, counts)] + [np.zeros(0, dtype=np.int64)])
            assert np.array_equal(on.data[found], values) and np.array_equal(rrow.data[found], where[values])
            if join_type == LEFT:
                valid = rrow.valid if rrow.valid is not None else np.ones(len(rrow), dtype=bool)      # Column drops a bitmap of all ones
                assert not valid[~found].any() and not rrow.data[~found].any() and valid[found].all()
        if "without a match" in name:
            assert pair.check([], [], 0, 1, 0, (False, False, INNER), [2], [1], name)[1]["output_rows"] == 10   # they vanish
            assert pair.check([], [], 0, 1, 0, (False, False, LEFT), [2], [1], name)[1]["output_rows"] == TILE + 60
    finally:
        pair.free()


# ---- 4. skew: one left row takes the whole right side ------------------------------------------------------------------------------
WIDE = {D: (-INF, INF), I64: (-(2 ** 63), 2 ** 63 - 1), I32: (-(2 ** 31), 2 ** 31 - 1)}


@pytest.mark.parametrize("t", [D, I64], ids=["DOUBLE", "INT64"])
def test_one_left_row_takes_the_whole_right_side(gpu_ctx, t):
    rng = np.random.default_rng(930 + int(t))
    nr = SWEEP + 2 * 64 + 78
    on = (rng.permutation(nr) - nr // 2).astype(NP[t])
    pair = Pair(gpu_ctx, [Column(t, np.array([WIDE[t][0]], dtype=NP[t])), Column(t, np.array([WIDE[t][1]], dtype=NP[t]))],
                [Column(t, on), Column(I32, np.arange(nr, dtype=np.int32))])
    try:
        for join_type in (INNER, LEFT):
            want, stats = pair.check([], [], 0, 1, 0, (False, False, join_type), [0], [0, 1], "one wide row")
            assert stats == {"left_rows": 1, "right_rows": nr, "output_rows": nr, "longest": nr}
            assert np.array_equal(want[1].data, np.sort(on)) and np.array_equal(want[2].data, np.argsort(on))   # the right side sorted by on
        assert pair.check([], [], 0, 1, 0, (True, True, SEMI), [0], [], "one wide row")[1]["output_rows"] == 1
    finally:
        pair.free()


def test_seventy_wide_rows_among_rows_that_match_nothing(gpu_ctx):
    rng = np.random.default_rng(935)
    nr, nl = SWEEP + 2 * 64 + 78, 300
    on = (rng.permutation(nr) - nr // 2).astype(np.int32)
    wide = np.zeros(nl, dtype=bool)
    wide[rng.permutation(nl)[:70]] = True
    lo = np.where(wide, WIDE[I32][0], 5).astype(np.int32)
    hi = np.where(wide, WIDE[I32][1], 4).astype(np.int32)
    pair = Pair(gpu_ctx, [Column(I32, lo), Column(I32, hi), Column(I32, np.arange(nl, dtype=np.int32))], [Column(I32, on)])
    try:
        want, stats = pair.check([], [], 0, 1, 0, (False, False, INNER), [2], [0], "seventy wide rows")
        assert stats == {"left_rows": nl, "right_rows": nr, "output_rows": 70 * nr, "longest": nr}
        assert np.array_equal(want[0].data, np.repeat(np.nonzero(wide)[0], nr)) and np.array_equal(want[1].data, np.tile(np.sort(on), 70))
    finally:
        pair.free()


# ---- 5. ties and strictness ------------------------------------------------------------------------------------------------------
def test_ties_and_strictness(gpu_ctx):
    """100 right rows hold on = 5, 3 hold 4 and 4 hold 6; 70 left rows ask for [5, 5], others for [4, 5], [5, 6] and [4, 6].
    A strict end drops exactly the rows equal to it; the rows of one value come in right row order."""
    rng = np.random.default_rng(940)
    ron = np.concatenate([np.full(100, 5), np.full(3, 4), np.full(4, 6)]).astype(np.int64)
    ron = ron[rng.permutation(len(ron))]
    asks = [(5, 5)] * 70 + [(4, 5), (5, 6), (4, 6)] * 2
    asks = [asks[i] for i in rng.permutation(len(asks))]
    have = {4: 3, 5: 100, 6: 4}
    for nby in (0, 1):
        by = [Column(B, np.ones(len(asks), dtype=bool))] * nby, [Column(B, np.ones(len(ron), dtype=bool))] * nby
        lcols = by[0] + [Column(I64, np.array([a for a, _ in asks], dtype=np.int64)), Column(I64, np.array([b for _, b in asks], dtype=np.int64))]
        pair = Pair(gpu_ctx, lcols, by[1] + [Column(I64, ron), Column(I64, np.arange(len(ron), dtype=np.int64))])
        try:
            for ls, hs in STRICTS:
                want, stats = pair.check(list(range(nby)), list(range(nby)), nby, nby + 1, nby, (ls, hs, INNER), [nby, nby + 1], [nby, nby + 1], f"ties nby {nby}")
                at = 0
                for a, b in asks:
                    values = [v for v in (4, 5, 6) if (v > a or (v == a and not ls)) and (v < b or (v == b and not hs))]
                    rows = np.concatenate([np.nonzero(ron == v)[0] for v in values] + [np.zeros(0, dtype=np.int64)])   # by value, then right row
                    assert sum(have[v] for v in values) == len(rows)
                    assert np.array_equal(want[3].data[at:at + len(rows)], rows), (ls, hs, a, b)
                    assert (want[0].data[at:at + len(rows)] == a).all() and (want[1].data[at:at + len(rows)] == b).all()
                    at += len(rows)
                assert at == stats["output_rows"] and stats["longest"] == (107 if not ls and not hs else 104 if not hs else 103 if not ls else 100)
        finally:
            pair.free()


# ---- 6. equality written as a range: the hash join's pairs, byte for byte ------------------------------------------------------------
HASH_KEYS = {I32: [7, -1, 0, 2 ** 31 - 1, -(2 ** 31), 12, 13], I64: [2 ** 53, 2 ** 53 + 1, -(2 ** 63), 2 ** 63 - 1, 0, 5, 6],
             D: [NAN, -0.0, 0.0, INF, -INF, 1.5, 2.5]}


@pytest.mark.parametrize("t", [I32, I64, D], ids=["INT32", "INT64", "DOUBLE"])
def test_equality_as_a_range_equals_the_hash_join(gpu_ctx, t):
    rng = np.random.default_rng(950 + int(t))
    nl, nr = T + 11, T // 2 + 70
    pool = np.array(HASH_KEYS[t], dtype=NP[t])
    if t == D:                                             # NaNs of several payloads: one key value, each row keeps its own bits
        pool = np.concatenate([pool, np.array([0x7ff8000000000001, 0xfff8000000000000], dtype=np.uint64).view(np.float64)])
    share = np.full(len(pool), 0.5 / (len(pool) - 1))
    share[0] = 0.5                                         # a heavy hitter: half of either side (NaN, for DOUBLE)
    lcols = [Column(t, pool[rng.choice(len(pool), nl, p=share)])] + payload(rng, nl)
    rpick = rng.choice(len(pool), nr, p=share)
    rcols = [Column(t, pool[np.where(rpick == 5, 6, rpick)])] + payload(rng, nr)                 # one key only the left holds: ANTI keeps rows
    pair = Pair(gpu_ctx, lcols, rcols)
    table = gpu_ctx.join_build(pair.rres, [0])
    try:
        for join_type in JOINS:
            right_out = [1, 2, 0] if join_type in (INNER, LEFT) else []
            hashed = table.probe(pair.lres, [0], join_type, [1, 0, 2], right_out)
            ranged = gpu_ctx.range_join(pair.lres, pair.rres, [], [], 0, 0, 0, False, False, join_type, [1, 0, 2], right_out)
            try:
                assert ranged.count == hashed.count > 0 and nullable_of(ranged) == nullable_of(hashed)
                assert column_bytes(ranged) == column_bytes(hashed), JOIN_NAMES[join_type]
                if join_type == INNER:
                    assert ranged.count > nl * nr // 5 and gpu_ctx.last_range_stats()["longest"] > nr // 3
            finally:
                hashed.free()
                ranged.free()
            pair.check([], [], 0, 0, 0, (False, False, join_type), [1, 0, 2], right_out, "equality")
    finally:
        table.free()
        pair.free()


def test_the_joins_agree_on_a_string_by_and_a_double_value(gpu_ctx):
    """The hash join on (by, value) against the range join with lo == hi == value, both ends inclusive, over one pair of
    results: the two share their argument checks and their output step, and equality of hash keys is ``Double.compareTo``
    equality (every NaN one value, -0.0 and 0.0 two).  300 left and 700 right rows: partial last bitmap words on both sides, a
    by dictionary that is translated, and more than two expansion tiles of INNER output."""
    rnd = random.Random(7)
    by_pool, value_pool = [None, "a", "b", "c"], [None, NAN, -0.0, 0.0, 1.5, -2.25, 3.0, INF]

    def side(n, dictionary):
        rows = [(rnd.choice(by_pool), rnd.choice(value_pool)) for _ in range(n)]
        by = Column(S, np.array([0 if b is None else dictionary.index(b) for b, _ in rows], dtype=np.int32),
                    np.array([b is not None for b, _ in rows]), dictionary)
        value = Column(D, np.array([0.0 if v is None else v for _, v in rows]), np.array([v is not None for _, v in rows]))
        return [by, value, Column(I64, np.arange(n, dtype=np.int64))]

    pair = Pair(gpu_ctx, side(300, ["a", "b", "c"]), side(700, ["c", "a", "b"]))      # two dictionary objects, two orders
    table = gpu_ctx.join_build(pair.rres, [0, 1])
    try:
        for join_type, rows in zip(JOINS, (4122, 4228, 194, 106)):                    # what the host operators give for these rows
            right_out = [2, 1, 0] if join_type in (INNER, LEFT) else []
            hashed = table.probe(pair.lres, [0, 1], join_type, [2, 0, 1], right_out)
            ranged = gpu_ctx.range_join(pair.lres, pair.rres, [0], [0], 1, 1, 1, False, False, join_type, [2, 0, 1], right_out)
            try:
                assert ranged.count == hashed.count == rows, JOIN_NAMES[join_type]
                assert join_type != INNER or ranged.count > 2 * TILE
                assert nullable_of(ranged) == nullable_of(hashed)
                assert [c.dictionary for c in ranged.to_columns()] == [c.dictionary for c in hashed.to_columns()]
                assert column_bytes(ranged) == column_bytes(hashed), JOIN_NAMES[join_type]         # row for row, bit for bit
            finally:
                hashed.free()
                ranged.free()
    finally:
        table.free()
        pair.free()


# ---- 7. special values of lo, hi and on --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [D, I64, I32], ids=["DOUBLE", "INT64", "INT32"])
def test_special_values_of_the_value_columns(gpu_ctx, t):
    rng = np.random.default_rng(960 + int(t))
    nl, nr = 333, 290
    pool = np.array(ON_SPECIALS[t], dtype=NP[t])
    if t == I64:
        assert len(set(pool.astype(np.float64))) < len(pool)                                 # pairs equal as doubles, different as integers
    draw = lambda n: Column(t, pool[rng.integers(0, len(pool), n)])                           # noqa: E731
    lcols = [Column(I32, rng.integers(0, 3, nl).astype(np.int32)), draw(nl), draw(nl)] + payload(rng, nl)
    rcols = [Column(I32, rng.integers(0, 3, nr).astype(np.int32)), draw(nr)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            _, stats = pair.check([0], [0], 1, 2, 1, form, [1, 2, 3], [1, 2], f"special {t.name}")
            assert 0 < stats["output_rows"] and stats["longest"] > 10
        for form in FORMS[:8]:
            pair.check([0], [0], 1, 1, 1, form, [1, 3], [1, 2], f"special {t.name}, lo is hi")
    finally:
        pair.free()


# ---- 8. NULLs ----------------------------------------------------------------------------------------------------------------------
def test_nulls_match_nothing_and_hide_nothing(gpu_ctx):
    rng = np.random.default_rng(970)
    nl, nr = 3 * 64 + 7, 2 * 64 + 50
    lcols = [with_nulls(Column(I32, rng.integers(0, 4, nl).astype(np.int32)), rng, 0.2)] + bounds(I32, rng, nl, 6, 0.2) + payload(rng, nl)
    rcols = [with_nulls(Column(I32, rng.integers(0, 4, nr).astype(np.int32)), rng, 0.2), value_column(I32, rng, nr, 6, 0.25)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        no_key = ~(lcols[0].valid & lcols[1].valid & lcols[2].valid)
        assert no_key.sum() > 40
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 2, 1, form, [3, 0, 1, 2], [0, 1, 2], "nulls")
            rows = want[0].data
            if form[2] in (INNER, SEMI):
                assert not no_key[rows].any()                                                   # a NULL by, lo or hi: no match
            if form[2] in (LEFT, ANTI):
                assert np.isin(np.nonzero(no_key)[0], rows).all()                               # .. and ANTI keeps those rows
            if form[2] == INNER:
                assert want[4].valid.all() and want[5].valid.all() and stats["output_rows"] > 100   # a match has a whole key
            if form[2] == LEFT:
                assert not want[6].valid[no_key[rows]].any()
    finally:
        pair.free()
    # a NULL `on` is not returned and does not hide the valid rows around it
    rcols = [Column(I32, np.array([1, 2, 3, 2], dtype=np.int32), np.array([True, False, True, True])), Column(I64, np.arange(4, dtype=np.int64))]
    lcols = [Column(I32, np.array([0, 2, 0], dtype=np.int32), np.array([True, True, False])), Column(I32, np.array([5, 2, 5], dtype=np.int32))]
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        want, _ = pair.check([], [], 0, 1, 0, (False, False, LEFT), [1], [1], "null on")
        assert np.where(want[1].valid, want[1].data, -1).tolist() == [0, 3, 2, 3, -1]
    finally:
        pair.free()


# ---- 9. by keys of every type --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nby", list(BY_SETS))
def test_by_columns_of_every_type(gpu_ctx, nby):
    rng = np.random.default_rng(980 + nby)
    nl, nr = 2 * T + 19, T + 45
    types = BY_SETS[nby]

    def by(n):
        ids = rng.integers(0, 40, n)
        return [with_nulls(by_column(t, ids, k), rng, 0.05) for k, t in enumerate(types)]
    pair = Pair(gpu_ctx, by(nl) + bounds(D, rng, nl, 30, 0.1, 12) + payload(rng, nl), by(nr) + [value_column(D, rng, nr, 30)] + payload(rng, nr))
    try:
        for form in FORMS:
            _, stats = pair.check(list(range(nby)), list(range(nby)), nby, nby + 1, nby, form, [nby + 2], [nby + 1, nby + 2], f"nby {nby}")
            assert stats["output_rows"] > nl // 4
    finally:
        pair.free()


@pytest.mark.parametrize("mode", list(DICTS))
def test_string_by_columns_compare_by_string(gpu_ctx, mode):
    rng = np.random.default_rng(990 + list(DICTS).index(mode))
    ld, rd = DICTS[mode]
    nl, nr = 200, 263
    lcols = [Column(S, rng.integers(0, len(ld), nl).astype(np.int32), rng.random(nl) > 0.1, ld)] + bounds(I32, rng, nl) + payload(rng, nl)
    rcols = [Column(S, rng.integers(0, len(rd), nr).astype(np.int32), rng.random(nr) > 0.1, rd), value_column(I32, rng, nr)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 2, 1, form, [0, 3], [0, 2], mode)
            assert want[0].dictionary == list(ld) and stats["output_rows"] > 0                  # each column its source's dictionary
            if form[2] == INNER:
                assert want[2].dictionary == list(rd)
                assert [ld[c] for c in want[0].data] == [rd[c] for c in want[2].data]            # the same string under whatever code
    finally:
        pair.free()


def test_double_by_columns_nan_and_signed_zero(gpu_ctx):
    rng = np.random.default_rng(1000)
    nl, nr = 150, 170
    nans = np.array([0x7ff8000000000000, 0x7ff8000000000001, 0xfff8000000000000], dtype=np.uint64).view(np.float64)
    pool = np.concatenate([nans, [-0.0, 0.0, INF]])
    lcols = [Column(D, pool[rng.integers(0, 6, nl)])] + bounds(I64, rng, nl) + payload(rng, nl)
    rcols = [Column(D, pool[rng.integers(0, 6, nr)]), value_column(I64, rng, nr)] + payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 2, 1, form, [0], [0, 2], "double by")
            if form[2] == INNER:                                                                # every NaN one value, -0.0 is not 0.0
                assert stats["output_rows"] > 100 and np.array_equal(np.isnan(want[0].data), np.isnan(want[1].data))
                real = ~np.isnan(want[0].data)
                assert np.array_equal(np.signbit(want[0].data[real]), np.signbit(want[1].data[real]))
    finally:
        pair.free()


# ---- 10. more than one sweep of the kernels --------------------------------------------------------------------------------------------
def test_one_partition_past_one_sweep(gpu_ctx):
    """No by column, n > SWEEP distinct values: the right rows hold the even ones, left row i asks for [2 i + 1, 2 i + 5], so its
    matches are known without the reference: the values 2 i + 2 and 2 i + 4."""
    rng = np.random.default_rng(1010)
    n = SWEEP + 2 * 64 + 78
    assert n > SWEEP and n % 2 == 0 and n % 64
    ron = np.arange(0, n, 2, dtype=np.int64)
    ron = ron[rng.permutation(len(ron))]
    lo = np.arange(1, n, 2, dtype=np.int64)
    lo = lo[rng.permutation(len(lo))]
    pair = Pair(gpu_ctx, [Column(I64, lo), Column(I64, lo + 4)], [Column(I64, ron), Column(I64, np.arange(len(ron), dtype=np.int64))])
    try:
        for form in ((False, False, INNER), (True, True, LEFT), (False, True, SEMI), (True, False, ANTI)):
            want, stats = pair.check([], [], 0, 1, 0, form, [0], [0, 1], "one partition past one sweep")
            assert stats["longest"] == 2 and stats["left_rows"] == stats["right_rows"] == n // 2
            if form[2] == INNER:
                values = np.stack([lo + 1, lo + 3], axis=1).reshape(-1)
                there = values <= n - 2                                                 # the two greatest left rows find one row or none
                assert stats["output_rows"] == there.sum() == 2 * (n // 2) - 3
                assert np.array_equal(want[0].data, np.repeat(lo, 2)[there]) and np.array_equal(want[1].data, values[there])
                assert np.array_equal(ron[want[2].data], want[1].data)
    finally:
        pair.free()


def test_many_partitions_past_one_sweep(gpu_ctx):
    rng = np.random.default_rng(1020)
    nl, nr = SWEEP // 2 + 4001, SWEEP // 2 + 77
    lcols = [Column(I32, rng.integers(0, 3000, nl).astype(np.int32))] + bounds(D, rng, nl, 50, 0.02, 8) + [Column(I64, np.arange(nl, dtype=np.int64))]
    rcols = [Column(I32, rng.integers(0, 3000, nr).astype(np.int32)), value_column(D, rng, nr, 50, 0.02), Column(I64, np.arange(nr, dtype=np.int64))]
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in ((False, False, INNER), (True, False, LEFT), (False, True, ANTI)):
            _, stats = pair.check([0], [0], 1, 2, 1, form, [3, 1], [2, 1], "many partitions past one sweep")
            assert 0 < stats["output_rows"] < nl if form[2] == ANTI else stats["output_rows"] > nl // 2
            assert 2 < stats["longest"] < 100
    finally:
        pair.free()


# ---- 11. degenerate inputs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", ["left", "right", "both"])
def test_empty_sides(gpu_ctx, empty):
    rng = np.random.default_rng(1030)
    n = 130
    full = [by_column(S, rng.integers(0, 5, n)), value_column(D, rng, n)] + payload(rng, n)
    none = [Column(c.type, c.data[:0], None, c.dictionary) for c in full]
    lcols, rcols = (none if empty in ("left", "both") else full), (none if empty in ("right", "both") else list(full))
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 1, 1, form, [0, 1, 3], [2, 3, 0], f"{empty} empty")
            keeps_left = empty == "right" and form[2] in (LEFT, ANTI)
            assert stats["output_rows"] == len(want[0].data) == (n if keeps_left else 0) and stats["longest"] == 0
            if form[2] in (INNER, LEFT):
                assert len(want) == 6 and want[5].dictionary == STRINGS
                assert [w.nullable for w in want[3:]] == ([True] * 3 if form[2] == LEFT else [False, bool(empty == "left"), False])
            else:
                assert len(want) == 3
    finally:
        pair.free()


def test_self_join_lists_and_nullability(gpu_ctx):
    rng = np.random.default_rng(1040)
    n = 2 * T + 3
    cols = [by_column(I32, rng.integers(0, 30, n))] + bounds(I64, rng, n, 40, 0.05) + payload(rng, n)
    pair = Pair(gpu_ctx, cols, cols)                  # the same handle on both sides
    try:
        for form in FORMS:
            want, stats = pair.check([0], [0], 1, 2, 1, form, [3, 1], [3, 1], "self")
            if form == (False, False, INNER):         # lo <= on(r) = lo(r) <= hi
                assert stats["output_rows"] > n and (want[3].data >= want[1].data).all()
        for form in ((False, False, LEFT), (True, True, INNER)):
            pair.check([0], [0], 1, 2, 1, form, [3, 3, 4, 3], [4, 4], "a column listed twice")
            pair.check([0], [0], 1, 2, 1, form, [], [3, 4], "no left column")
            pair.check([0], [0], 1, 2, 1, form, [4, 3], [], "no right column")
            pair.check([0, 0], [0, 0], 1, 2, 1, form, [3], [3], "a by column listed twice")
        want, _ = pair.check([0], [0], 1, 2, 1, (False, False, LEFT), [0, 3], [0, 3], "nullability")
        assert [w.nullable for w in want] == [False, False, True, True]                       # LEFT: every right column nullable
        want, _ = pair.check([0], [0], 1, 2, 1, (False, False, INNER), [0, 3, 4], [0, 3, 4], "nullability")
        assert [w.nullable for w in want] == [False, False, True] * 2                         # INNER: the source's
        want, _ = pair.check([0], [0], 1, 2, 1, (False, False, ANTI), [0, 1, 4], [], "nullability")
        assert [w.nullable for w in want] == [False, True, True]
    finally:
        pair.free()


# ---- 12. composition ------------------------------------------------------------------------------------------------------------------
def test_bounds_made_by_a_projection(gpu_ctx):
    """`t - 2.5` and `t + 2.5` computed by qe_filter_project and fed straight in: the quotes around every trade."""
    ctx = gpu_ctx
    rng = np.random.default_rng(1050)
    nl, nr = T + 9, 3 * T + 1
    sym = ["x", "y", "z"]
    trades = [Column(S, rng.integers(0, 3, nl).astype(np.int32), None, sym), Column(D, rng.integers(0, 4000, nl) / 4.0)]
    quotes = [Column(S, rng.integers(0, 3, nr).astype(np.int32), None, sym), Column(D, rng.integers(0, 4000, nr) / 4.0), Column(I64, np.arange(nr, dtype=np.int64))]
    t = ColumnExpression("t", 1, D)
    shifted = lambda fn: FunctionExpression(fn, [t, NumericLiteralExpression(2.5)], D)      # noqa: E731
    batch = E.DeviceBatch.from_columns(ctx, trades)
    lres = E.filter_project(ctx, batch, None, [ctx.compile(e) for e in (ColumnExpression("s", 0, S), t, shifted(Function.SUB), shifted(Function.ADD))])
    rbatch, rres = build(ctx, quotes)
    lcols = trades + [Column(D, trades[1].data - 2.5), Column(D, trades[1].data + 2.5)]
    try:
        for form in ((False, False, INNER), (False, True, LEFT)):
            want, stats = range_reference(lcols, quotes, nullable_of(lres), nullable_of(rres), [0], [0], 2, 3, 1, *form, [0, 1], [1, 2])
            out = ctx.range_join(lres, rres, [0], [0], 2, 3, 1, *form, [0, 1], [1, 2])
            assert ctx.last_range_stats() == stats and stats["output_rows"] > 2 * nl
            assert_window_output(out, want, "projected bounds")
            ok = want[2].valid
            assert (np.abs(want[2].data[ok] - want[1].data[ok]) <= 2.5).all()
            out.free()
    finally:
        for r in (lres, batch, rres, rbatch):
            r.free()


def test_the_output_is_an_ordinary_result(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(1060)
    nl, nr = 2 * T + 5, T + 71
    lcols = [by_column(I32, rng.integers(0, 9, nl))] + bounds(D, rng, nl, 40) + payload(rng, nl)
    rcols = [by_column(I32, rng.integers(0, 9, nr)), value_column(D, rng, nr, 40)] + payload(rng, nr)
    pair = Pair(ctx, lcols, rcols)
    want, _ = range_reference(lcols, rcols, nullable_of(pair.lres), nullable_of(pair.rres), [0], [0], 1, 2, 1, False, False, LEFT, [3, 1], [2, 1])
    out = ctx.range_join(pair.lres, pair.rres, [0], [0], 1, 2, 1, False, False, LEFT, [3, 1], [2, 1])
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
    host = [Column(w.type, w.data, w.valid if w.nullable else None, w.dictionary) for w in want]
    second_want, stats = range_reference(host, host, [w.nullable for w in want], [w.nullable for w in want], [], [], 0, 0, 2, False, False, SEMI, [0, 2], [])
    second = ctx.range_join(out, out, [], [], 0, 0, 2, False, False, SEMI, [0, 2], [])          # and into another range join, with itself:
    assert ctx.last_range_stats() == stats and 0 < second.count < out.count                     # the left rows whose id is some row's matched id
    assert_window_output(second, second_want, "a second range join")
    for r in (second, by_rid, again, batch, out):
        r.free()


# ---- 13. the operator ------------------------------------------------------------------------------------------------------------------
def test_operator_on_gpu_sources_matches_its_host_branch(gpu_ctx):
    from queryengine_amd import ColumnarTable, Field, Schema
    from queryengine_amd.operators import GpuFilterProjectOperator, RangeJoinOperator, map as op_map
    from test_setop_cpu import Rows, assert_rows
    rng = np.random.default_rng(1070)
    values = np.array([NAN, -0.0, 0.0, 1.5, -INF, INF, 3.0])

    def table(n, dictionary, nvalues):
        cols = [Column(S, rng.integers(0, len(dictionary), n).astype(np.int32), rng.random(n) > 0.2, dictionary)]
        cols += [Column(D, values[rng.integers(0, len(values), n)], rng.random(n) > 0.2) for _ in range(nvalues)]
        cols.append(Column(I64, np.arange(n, dtype=np.int64)))
        names = ["k"] + [f"v{i}" for i in range(nvalues)] + ["id"]
        return cols, ColumnarTable(Schema([Field(name, c.type) for name, c in zip(names, cols)]), cols), names
    (lcols, ltable, lnames), (rcols, rtable, rnames) = table(150, ["a", "b", "c"], 2), table(170, ["c", "d", "a"], 1)
    exprs = lambda cols, names: [ColumnExpression(name, i, c.type) for i, (name, c) in enumerate(zip(names, cols))]      # noqa: E731
    boxed = lambda cols, n: [[c.value(i) for c in cols] for i in range(n)]      # noqa: E731
    for lo_strict, hi_strict, join_type in FORMS:
        left = GpuFilterProjectOperator(gpu_ctx, ltable.getScanOperator(lnames), None, exprs(lcols, lnames))
        right = GpuFilterProjectOperator(gpu_ctx, rtable.getScanOperator(rnames), None, exprs(rcols, rnames))
        dev = op_map(RangeJoinOperator(left, right, [0], [0], 1, 2, 1, lo_strict, hi_strict, join_type), list)
        host = op_map(RangeJoinOperator(Rows(boxed(lcols, 150)), Rows(boxed(rcols, 170)), [0], [0], 1, 2, 1, lo_strict, hi_strict, join_type,
                                        right_out=[0, 1, 2] if join_type in (INNER, LEFT) else None), list)
        assert_rows(dev, host, f"strict {lo_strict} {hi_strict} join {join_type}")
        assert len(host) > 5


# ---- 14. determinism -------------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_on_every_run_and_on_a_fresh_context(gpu_ctx):
    rng = np.random.default_rng(1080)
    nl, nr = 3 * T + 5, 2 * T + 71
    lcols = [with_nulls(by_column(S, rng.integers(0, 9, nl)), rng), by_column(D, rng.integers(0, 5, nl))] + bounds(D, rng, nl, 40) + payload(rng, nl)
    rcols = [with_nulls(by_column(S, rng.integers(0, 9, nr), 0, STRINGS[::-1]), rng), by_column(D, rng.integers(0, 5, nr)), value_column(D, rng, nr, 40)] + payload(rng, nr)

    def run(ctx):
        pair = Pair(ctx, lcols, rcols)
        data = []
        for lo_strict, hi_strict, join_type in FORMS:
            out = ctx.range_join(pair.lres, pair.rres, [0, 1], [0, 1], 2, 3, 2, lo_strict, hi_strict, join_type, [4, 5, 2],
                                 [3, 4, 2, 0] if join_type in (INNER, LEFT) else [])
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


# ---- 15. the errors that need a result to look at -----------------------------------------------------------------------------------
def test_invalid_arguments(gpu_ctx):
    ctx = gpu_ctx
    lib = ctx._lib
    rng = np.random.default_rng(1090)
    n = 50
    cols = [Column(I32, rng.integers(0, 5, n).astype(np.int32)), Column(D, rng.normal(0, 1, n)), Column(S, rng.integers(0, 3, n).astype(np.int32), None, STRINGS),
            Column(B, rng.random(n) > 0.5), Column(I64, np.arange(n, dtype=np.int64)), Column(D, rng.normal(0, 1, n) + 1.0)]
    pair = Pair(ctx, cols, cols)
    res = pair.lres

    def call(left_by=(0,), right_by=(0,), lo=1, hi=5, on=1, lo_strict=0, hi_strict=0, join_type=LEFT, left_out=(4,), right_out=(4,), null=()):
        out = C.c_void_p(0xdead)
        arr = lambda v: (C.c_int32 * max(1, len(v)))(*v)     # noqa: E731
        st = lib.qe_result_range_join(None if "ctx" in null else ctx.handle, None if "left" in null else res.handle, None if "right" in null else res.handle,
                                      arr(left_by), arr(right_by), len(left_by), lo, hi, on, lo_strict, hi_strict, join_type,
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
        for bad in (dict(left_by=(6,)), dict(right_by=(-1,)), dict(lo=6), dict(hi=-1), dict(on=6), dict(left_out=(6,)), dict(right_out=(4, -1)),   # out of range
                    dict(left_by=(0,), right_by=(4,)), dict(left_by=(0, 2), right_by=(0, 3)),                   # paired by columns of different types
                    dict(lo=2, hi=2, on=2), dict(lo=3, hi=3, on=3),                                             # value columns STRING, BOOLEAN
                    dict(lo=1, hi=5, on=4), dict(lo=1, hi=4, on=1), dict(lo=0, hi=1, on=1),                     # value types differ among the three
                    dict(left_by=tuple(range(5)) + (0, 1, 2), right_by=tuple(range(5)) + (0, 1, 2)),            # eight by columns
                    dict(lo_strict=2), dict(hi_strict=-1), dict(join_type=4), dict(left_out=(), right_out=()),
                    dict(join_type=SEMI), dict(join_type=ANTI, left_out=(), right_out=())):
            assert call(**bad) == INVALID_ARG, bad
        assert call(left_by=(), right_by=(), lo=4, hi=4, on=4) == N.OK and call(lo=0, hi=0, on=0) == N.OK
        assert call(left_by=tuple(range(5)) + (0, 2), right_by=tuple(range(5)) + (0, 2)) == N.OK               # seven by columns
        assert call(join_type=SEMI, right_out=()) == N.OK
        pair.check([0, 2, 3], [0, 2, 3], 1, 5, 1, (False, False, LEFT), [4], [4], "after the errors")          # the context still works
    finally:
        pair.free()
