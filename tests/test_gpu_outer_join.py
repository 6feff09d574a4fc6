"""RIGHT and FULL OUTER on the device: qe_join_probe and qe_result_range_join with QE_JOIN_RIGHT / QE_JOIN_FULL.

The expectation is tests/outer_join_reference.py (numpy; proved equal to the host branches of ``HashJoinOperator`` and
``RangeJoinOperator`` in tests/test_outer_join_cpu.py): the INNER / LEFT rows, then every build / right row nobody matched, in
row order, with NULL probe / left columns.  Every output column is compared in full -- type, nullable flag, dictionary,
validity, values by bits, zero under a "none" on EITHER side -- with no tolerance; counts, last_join_stats / last_range_stats
and last_outer_stats are checked too.  Sizes are those where the new device code changes path: the 64-row words of the
matched bitmap, the 1024-word blocks of its ranks (65 536 build rows), the 1024-element blocks of the scan over the range
join's difference array and the second trip of its block sums (2^20 + 1 eligible right rows), and the cases where many lanes
mark one build row or one bitmap word at once."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_columns_equal, col
from join_reference import assert_join_output, expected_columns, reference_pairs
from outer_join_reference import FULL, HASH_PROBE, RANGE_JOIN, RIGHT, hash_outer_pairs, outer_expected, range_outer_pairs
from queryengine_amd import AggregationFunction as AF
from queryengine_amd import Column, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N
from test_gpu_asof import build, column_bytes, nullable_of, with_nulls
from test_gpu_asof import payload as range_payload
from test_gpu_join import SIZES, as_side, payload, side_nullable
from test_gpu_range_join import STRICTS, Pair, bounds, value_column
from window_reference import assert_window_output

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
INNER, LEFT = N.JOIN_INNER, N.JOIN_LEFT
OUTER = [RIGHT, FULL]
NAMES = {RIGHT: "RIGHT", FULL: "FULL"}
INVALID_ARG = 1
NAN = float("nan")
NAN2 = np.array([0x7ff8000000000002], dtype=np.uint64).view(np.float64)[0]


# ---- the hash join ------------------------------------------------------------------------------------------------------------------
def probe_check(ctx, table, pside, bside, pcols, bcols, pk, bk, jt, probe_out, build_out, what=""):
    """One qe_join_probe under RIGHT / FULL against the reference; returns (prow, brow, outer stats)."""
    prow, brow, stats = hash_outer_pairs(pcols, bcols, pk, bk, jt)
    want = outer_expected(pcols, bcols, side_nullable(bside, bcols), prow, brow, probe_out, build_out, jt)
    res = table.probe(pside, pk, jt, probe_out, build_out)
    try:
        what = f"{what} {NAMES[jt]}"
        assert res.count == len(prow), (what, res.count, len(prow))
        assert_window_output(res, want, what)
        assert ctx.last_join_stats()[1:3] == [len(pcols[0]), len(prow)], (what, ctx.last_join_stats())
        assert ctx.last_outer_stats() == stats and stats[0] == HASH_PROBE and stats[2] + stats[3] == len(bcols[0]), (what, ctx.last_outer_stats(), stats)
    finally:
        res.free()
    return prow, brow, stats


def hash_case(ctx, pcols, bcols, pk, bk, kinds=("result", "result"), what="", probe_out=None, build_out=None):
    """Build + probe under RIGHT and FULL with every payload column and the first key in the output."""
    probe_out = (list(range(len(pk), len(pcols))) + [pk[0]]) if probe_out is None else probe_out
    build_out = (list(range(len(bk), len(bcols))) + [bk[0]]) if build_out is None else build_out
    pside, pfree = as_side(ctx, pcols, kinds[0])
    bside, bfree = as_side(ctx, bcols, kinds[1])
    table = ctx.join_build(bside, bk)
    try:
        return {jt: probe_check(ctx, table, pside, bside, pcols, bcols, pk, bk, jt, probe_out, build_out, what)[2] for jt in OUTER}
    finally:
        table.free()
        for h in pfree + bfree:
            h.free()


PDICT = ["x", "b", "a", "q", "～", "aa"]                     # "x", "q" only here
BDICT = ["aa", "a", "zz", "b", "～", "a", "Zü"]              # "zz", "Zü" only here; "a" listed twice
DOUBLE_KEYS = np.array([NAN, NAN2, -0.0, 0.0, 1.5, -2.25])


def key_columns(kind, rng, n, build_side):
    """20 % NULL keys; few distinct values, so that duplicate keys meet across the sides and some build keys meet nothing."""
    def nulls(c):
        return Column(c.type, c.data, rng.random(n) >= 0.2 if n else None, c.dictionary)
    if kind == "int64":
        return [nulls(Column(I64, rng.integers(0, max(4, n // 2 + 3), n).astype(np.int64) * (2 ** 40 + 1)))]
    if kind == "string-double":
        d = BDICT if build_side else PDICT
        return [nulls(Column(S, rng.integers(0, len(d), n).astype(np.int32), None, d)), nulls(Column(D, DOUBLE_KEYS[rng.integers(0, 6, n)]))]
    return [nulls(Column(B, rng.random(n) > 0.5)), nulls(Column(I32, rng.integers(-3, max(4, n // 8), n).astype(np.int32)))]


@pytest.mark.parametrize("kind", ["int64", "string-double", "boolean-int32"])
@pytest.mark.parametrize("case", range(len(SIZES)), ids=[f"{p}x{b}" for p, b in SIZES])
def test_right_and_full_at_every_size(gpu_ctx, case, kind):
    np_, nb = SIZES[case]
    rng = np.random.default_rng([70, case, len(kind)])
    pcols = key_columns(kind, rng, np_, False) + payload(rng, np_, False)
    bcols = key_columns(kind, rng, nb, True) + payload(rng, nb, True)
    nk = len(pcols) - 2
    stats = hash_case(gpu_ctx, pcols, bcols, list(range(nk)), list(range(nk)), ("batch", "result") if case % 2 else ("result", "batch"), f"{kind} {np_}x{nb}")
    assert stats[RIGHT][2:] == stats[FULL][2:]                                   # one tail
    if np_ == 0:
        assert stats[FULL][1:] == [0, nb, 0]                                     # the tail is the whole build side
    if nb == 0:
        assert stats[RIGHT][1:] == [0, 0, 0] and stats[FULL][1:] == [np_, 0, 0]  # RIGHT is empty, FULL is LEFT
    if min(np_, nb) > 60:
        assert stats[RIGHT][2] > 0 and stats[RIGHT][3] > 0


@pytest.mark.parametrize("nb", [64, 65, 128, 65535, 65536, 65537])
def test_bitmap_seams(gpu_ctx, nb):
    """The only matched build row is row 0, 63, 64 or the last; every row; no row; and a table of 0 rows (every key NULL)."""
    ctx = gpu_ctx
    rng = np.random.default_rng(7100 + nb)
    key = rng.permutation(nb).astype(np.int64)                                   # distinct: build row r holds key[r]
    bcols = [Column(I64, key), Column(I64, np.arange(nb, dtype=np.int64)), Column(I32, rng.integers(-5, 5, nb).astype(np.int32))]
    bside, bfree = as_side(ctx, bcols, "result")
    table = ctx.join_build(bside, [0])
    probes = {f"row {r}": np.array([key[r], key[r]], dtype=np.int64) for r in (0, 63, min(64, nb - 1), nb - 1)}
    probes["every row"] = key[rng.permutation(nb)]
    probes["no row"] = np.array([-1, nb, -7], dtype=np.int64)
    try:
        for name, pk in probes.items():
            pcols = [Column(I64, pk), Column(I64, np.arange(len(pk), dtype=np.int64))]
            pside, pfree = as_side(ctx, pcols, "batch")
            for jt in OUTER:
                _, brow, stats = probe_check(ctx, table, pside, bside, pcols, bcols, [0], [0], jt, [1], [1, 2], f"nb {nb} {name}")
                tail = brow[stats[1]:]
                if name.startswith("row "):
                    assert tail.tolist() == [r for r in range(nb) if r != int(name[4:])]
                assert stats[2] == {"every row": 0, "no row": nb}.get(name, nb - 1)
            for h in pfree:
                h.free()
    finally:
        table.free()
        for h in bfree:
            h.free()
    nulls = [Column(I64, key, np.zeros(nb, dtype=bool))] + bcols[1:]
    stats = hash_case(ctx, [Column(I64, key[:50]), Column(I64, np.arange(50, dtype=np.int64))], nulls, [0], [0], what=f"nb {nb} every key NULL")
    assert stats[RIGHT][1:] == [0, nb, 0] and stats[FULL][1:] == [50, nb, 0]


def test_many_lanes_mark_one_build_row_and_one_word(gpu_ctx):
    rng = np.random.default_rng(72)
    ids = lambda n: Column(I64, np.arange(n, dtype=np.int64))                    # noqa: E731
    # 8192 probe rows all equal to ONE build key
    bcols = [Column(I32, np.arange(100, dtype=np.int32)), ids(100)]
    stats = hash_case(gpu_ctx, [Column(I32, np.full(8192, 37, dtype=np.int32)), ids(8192)], bcols, [0], [0], what="one build key")
    assert stats[RIGHT] == [HASH_PROBE, 8192, 99, 1]
    # the 64 build rows of one bitmap word, each hit by 128 probe rows (and a second word nobody hits)
    bcols = [Column(I32, np.arange(70, dtype=np.int32)), ids(70)]
    stats = hash_case(gpu_ctx, [Column(I32, rng.permutation(np.repeat(np.arange(64, dtype=np.int32), 128))), ids(8192)], bcols, [0], [0], what="one word")
    assert stats[FULL] == [HASH_PROBE, 8192, 6, 64]
    # one build key 300 times: every copy is matched, none is in the tail
    key = rng.permutation(np.concatenate([np.full(300, 5, dtype=np.int32), np.arange(100, 400, dtype=np.int32)]))
    stats = hash_case(gpu_ctx, [Column(I32, np.array([5, 9, 5], dtype=np.int32)), ids(3)], [Column(I32, key), ids(600)], [0], [0], what="300 copies")
    assert stats[RIGHT] == [HASH_PROBE, 600, 300, 300] and stats[FULL] == [HASH_PROBE, 601, 300, 300]


def test_the_marks_belong_to_the_call_not_to_the_table(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(73)
    nb = 500
    bcols = [Column(I64, np.arange(nb, dtype=np.int64) % 250)] + payload(rng, nb, True)
    a = [Column(I64, rng.integers(0, 100, 300))] + payload(rng, 300, False)       # A matches build keys below 100
    b = [Column(I64, rng.integers(80, 200, 300))] + payload(rng, 300, False)      # B matches 80 .. 199
    bside, bfree = as_side(ctx, bcols, "batch")
    aside, afree = as_side(ctx, a, "result")
    bs, bsfree = as_side(ctx, b, "result")
    table = ctx.join_build(bside, [0])
    try:
        probe_out, build_out = [1, 2, 0], [1, 2, 3, 4, 0]
        _, brow_a, st_a = probe_check(ctx, table, aside, bside, a, bcols, [0], [0], FULL, probe_out, build_out, "A")
        res = table.probe(bs, [0], INNER, probe_out, build_out)                   # an old type in between: the same bytes as ever
        prow, brow = reference_pairs(b, bcols, [0], [0], INNER)
        assert res.count == len(prow) and ctx.last_outer_stats() == st_a          # other join types leave the outer stats alone
        assert_join_output(res.to_columns(), expected_columns(b, bcols, prow, brow, probe_out, build_out, INNER), brow, len(probe_out), "B INNER")
        res.free()
        _, brow_b, st_b = probe_check(ctx, table, bs, bside, b, bcols, [0], [0], RIGHT, probe_out, build_out, "B")
        only_a = set(brow_a[:st_a[1]][brow_a[:st_a[1]] >= 0].tolist()) - set(brow_b[:st_b[1]].tolist())
        assert len(only_a) > 50 and only_a <= set(brow_b[st_b[1]:].tolist())     # what only A matched is in B's tail
    finally:
        table.free()
        for h in afree + bsfree + bfree:
            h.free()


def test_the_same_bytes_on_every_run_and_context_hash(gpu_ctx):
    rng = np.random.default_rng(74)
    np_, nb = 8009, 2003
    pcols = key_columns("int64", rng, np_, False) + payload(rng, np_, False)
    bcols = key_columns("int64", rng, nb, True) + payload(rng, nb, True)

    def run(ctx):
        pside, pfree = as_side(ctx, pcols, "batch")
        bside, bfree = as_side(ctx, bcols, "batch")
        table = ctx.join_build(bside, [0])
        res = table.probe(pside, [0], FULL, [0, 1, 2], [0, 1, 2, 3, 4])
        raw = column_bytes(res)
        for h in [res, table] + pfree + bfree:
            h.free()
        return raw

    first = run(gpu_ctx)
    assert len(first[0][0]) > 8 * np_ and run(gpu_ctx) == first
    other = E.Context(device=0)
    try:
        assert run(other) == first
    finally:
        other.close()


def test_a_full_join_feeds_the_next_plan(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(75)
    np_, nb = 3000, 400
    pcols = [Column(I32, rng.integers(0, 500, np_).astype(np.int32)), Column(I64, np.arange(np_, dtype=np.int64)),
             Column(S, rng.integers(0, 3, np_).astype(np.int32), rng.random(np_) > 0.1, ["u", "v", "w"]), Column(D, rng.integers(-9, 9, np_).astype(np.float64))]
    bcols = [Column(I32, rng.permutation(700)[:nb].astype(np.int32)), Column(I64, np.arange(nb, dtype=np.int64)),
             Column(I32, rng.integers(0, 4, nb).astype(np.int32), rng.random(nb) > 0.1), Column(D, rng.integers(-9, 9, nb).astype(np.float64))]
    pside, pfree = as_side(ctx, pcols, "batch")
    bside, bfree = as_side(ctx, bcols, "result")
    table = ctx.join_build(bside, [0])
    probe_out, build_out = [1, 2, 3], [2, 1, 3]        # probe row id, probe tag, probe value | build class, build row id, build value
    prow, brow, stats = hash_outer_pairs(pcols, bcols, [0], [0], FULL)
    assert stats[2] > 50 and (brow[:stats[1]] < 0).sum() > 50
    want = outer_expected(pcols, bcols, side_nullable(bside, bcols), prow, brow, probe_out, build_out, FULL)
    joined = table.probe(pside, [0], FULL, probe_out, build_out)
    hbatch, hres = build(ctx, [Column(w.type, w.data, w.valid, w.dictionary) for w in want])       # the reference rows, pinned
    try:
        assert_window_output(joined, want, "FULL")
        keys = [(3, False), (1, True), (0, False), (4, True)]      # (probe row id, build row id) is unique: a total order
        got, exp = ctx.order_by_keys(joined, keys, None), ctx.order_by_keys(hres, keys, None)
        assert got.count == exp.count == len(prow)
        for g, w in zip(got.to_columns(), exp.to_columns()):
            assert_columns_equal(g, w, "ORDER BY over the FULL join")
        got.free(); exp.free()
        jbatch = joined.as_batch()
        for key in (col("tag", 1, S), col("class", 3, I32)):                     # COUNT per key, NULL being a key value
            args = ([ctx.compile(key)], [ctx.compile(col("pv", 2, D)), ctx.compile(col("bv", 5, D))], [int(AF.COUNT), int(AF.COUNT)])
            got, exp = E.filter_groupby(ctx, jbatch, None, *args), E.filter_groupby(ctx, hbatch, None, *args)
            assert got.count == exp.count > 3
            for g, w in zip(got.to_columns(), exp.to_columns()):
                assert_columns_equal(g, w, "GROUP BY over the FULL join")
            assert got.to_columns()[0].valid is not None                          # a NULL group: the tail's (or the unmatched rows')
            got.free(); exp.free()
        jbatch.free()
    finally:
        for h in [joined, hres, hbatch, table] + pfree + bfree:
            h.free()


def test_invalid_arguments_of_the_probe(gpu_ctx, native_lib):
    lib, ctx = native_lib, gpu_ctx
    rng = np.random.default_rng(76)
    pcols = [Column(I64, rng.integers(0, 50, 300))] + payload(rng, 300, False)
    bcols = [Column(I64, rng.integers(0, 70, 100))] + payload(rng, 100, True)
    pside, pfree = as_side(ctx, pcols, "batch")
    bside, bfree = as_side(ctx, bcols, "result")
    table = ctx.join_build(bside, [0])
    pin = N.JoinInput(None, pside.handle)
    arr = lambda v: (C.c_int32 * 8)(*v)                                          # noqa: E731

    def probe(jt, pout, bout):
        out = C.c_void_p(0xdead)
        st = lib.qe_join_probe(ctx.handle, table.handle, C.byref(pin), arr([0]), 1, jt, arr(pout), len(pout), arr(bout), len(bout), C.byref(out))
        if st != N.OK:
            assert out.value is None
        else:
            lib.qe_result_free(ctx.handle, out)
        return st

    try:
        for jt in (5, 6, 7, 10):
            assert probe(jt, [1], [1]) == INVALID_ARG and b"unknown join type" in lib.qe_last_error(ctx.handle)
        assert probe(RIGHT, [], []) == INVALID_ARG and b"no output column" in lib.qe_last_error(ctx.handle)
        assert probe(RIGHT, [], [1]) == N.OK
        for jt in OUTER:                                                         # the context still works; no probe column at all
            probe_check(ctx, table, pside, bside, pcols, bcols, [0], [0], jt, [], [1, 0], "no probe column")
    finally:
        table.free()
        for h in pfree + bfree:
            h.free()


# ---- the range join -----------------------------------------------------------------------------------------------------------------
def range_check(pair, left_by, right_by, lo, hi, on, lo_strict, hi_strict, jt, left_out, right_out, what=""):
    """One qe_result_range_join under RIGHT / FULL against the reference; returns (lrow, rrow, outer stats)."""
    ctx = pair.ctx
    lrow, rrow, stats, longest = range_outer_pairs(pair.lcols, pair.rcols, left_by, right_by, lo, hi, on, lo_strict, hi_strict, jt)
    want = outer_expected(pair.lcols, pair.rcols, nullable_of(pair.rres), lrow, rrow, left_out, right_out, jt)
    out = ctx.range_join(pair.lres, pair.rres, left_by, right_by, lo, hi, on, lo_strict, hi_strict, jt, left_out, right_out)
    try:
        what = f"{what}: {'(' if lo_strict else '['}lo, hi{')' if hi_strict else ']'} {NAMES[jt]}"
        assert out.count == len(lrow), (what, out.count, len(lrow))
        assert_window_output(out, want, what)
        nl, nr = len(pair.lcols[0]), len(pair.rcols[0])
        assert ctx.last_range_stats() == {"left_rows": nl, "right_rows": nr, "output_rows": len(lrow), "longest": longest}, (what, ctx.last_range_stats())
        assert ctx.last_outer_stats() == stats and stats[0] == RANGE_JOIN and stats[2] + stats[3] == nr, (what, ctx.last_outer_stats(), stats)
    finally:
        out.free()
    return lrow, rrow, stats


LDICT, RDICT = ["b", "a", "", "zz", "q"], ["zz", "a", "x", "b"]                   # "", "q" only left; "x" only right


def by_columns(nby, rng, n, right_side):
    d = RDICT if right_side else LDICT
    cols = [Column(S, rng.integers(0, len(d), n).astype(np.int32), None, d), Column(I32, rng.integers(0, 3, n).astype(np.int32))][:nby]
    return [with_nulls(c, rng, 0.08) for c in cols]


@pytest.mark.parametrize("t", [D, I64, I32], ids=["DOUBLE", "INT64", "INT32"])
@pytest.mark.parametrize("nby", [0, 1, 2])
def test_range_right_and_full_by_and_value_types(gpu_ctx, nby, t):
    """NULLs in by, lo, hi and on; STRING by columns over different dictionaries; both strict flags."""
    rng = np.random.default_rng([80, nby, int(t)])
    nl, nr = 700, 523
    lcols = by_columns(nby, rng, nl, False) + bounds(t, rng, nl, 40, 0.1, 5) + range_payload(rng, nl)
    rcols = by_columns(nby, rng, nr, True) + [value_column(t, rng, nr, 40, 0.1)] + range_payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        by = list(range(nby))
        for jt in OUTER:
            for ls, hs in STRICTS:
                _, _, stats = range_check(pair, by, by, nby, nby + 1, nby, ls, hs, jt, [nby + 2, nby + 3, nby], [nby + 1, nby + 2, nby], f"nby {nby}")
                assert stats[2] > 20 and stats[3] > 20
        range_check(pair, by, by, nby, nby, nby, False, False, FULL, [nby + 2], [nby + 1], "lo == hi")          # one column as both bounds
        range_check(pair, by, by, nby, nby, nby, False, False, RIGHT, [], [nby + 1, nby + 1], "lo == hi, no left column")
    finally:
        pair.free()


def test_range_left_and_right_one_handle(gpu_ctx):
    rng = np.random.default_rng(81)
    n = 600
    cols = [Column(I32, rng.integers(0, 4, n).astype(np.int32))] + bounds(I64, rng, n, 30, 0.1, 4) + range_payload(rng, n)
    pair = Pair(gpu_ctx, cols, cols)
    try:
        for jt in OUTER:
            for ls, hs in ((False, False), (True, False)):
                _, _, stats = range_check(pair, [0], [0], 1, 2, 1, ls, hs, jt, [3, 1], [3, 4], "self")
                assert stats[2] > 0 and stats[3] > 0
    finally:
        pair.free()


def simple_pair(ctx, lo, hi, on):
    """nby = 0, INT32 values.  Left: lo, hi, row id; right: on, row id."""
    i32 = lambda v: Column(I32, np.asarray(v, dtype=np.int32))                   # noqa: E731
    return Pair(ctx, [i32(lo), i32(hi), i32(np.arange(len(lo)))], [i32(on), i32(np.arange(len(on)))])


def test_one_right_row_covered_by_5000_left_rows(gpu_ctx):
    rng = np.random.default_rng(82)
    on = rng.permutation(200)
    pair = simple_pair(gpu_ctx, np.full(5000, 77), np.full(5000, 77), on)
    try:
        for jt in OUTER:
            _, rrow, stats = range_check(pair, [], [], 0, 1, 0, False, False, jt, [2], [1], "5000 on one")
            assert stats == [RANGE_JOIN, 5000, 199, 1] and rrow[5000:].tolist() == [r for r in range(200) if on[r] != 77]
    finally:
        pair.free()


def test_adjacent_intervals(gpu_ctx):
    rng = np.random.default_rng(83)
    a, b, c = 10, 25, 40
    on = rng.permutation(np.arange(a + 1, c))                                    # a + 1 .. c - 1, b among them
    pair = simple_pair(gpu_ctx, [a, b], [b, c], on)
    try:
        for jt in OUTER:
            assert range_check(pair, [], [], 0, 1, 0, False, True, jt, [2], [1], "[a, b) [b, c)")[2][2] == 0            # nothing is left out
            _, rrow, stats = range_check(pair, [], [], 0, 1, 0, True, True, jt, [2], [1], "(a, b) (b, c)")
            assert stats[2] == 1 and on[rrow[-1]] == b                                                                   # exactly b
    finally:
        pair.free()


@pytest.mark.parametrize("edge", [1023, 1024, 1025])
def test_a_covered_run_ends_and_starts_at_the_scan_block(gpu_ctx, edge):
    """The right side holds the distinct values 0 .. 2999, so a value is its position in the list of right rows.  Positions
    0 .. edge - 1 and edge + 1 .. 2999 are covered: the cover count falls to 0 and rises again around one block edge of the scan."""
    rng = np.random.default_rng(84 + edge)
    on = rng.permutation(3000)
    pair = simple_pair(gpu_ctx, [0, edge + 1, 5], [edge - 1, 2999, 3], on)       # (the third interval is reversed: empty)
    try:
        for jt in OUTER:
            _, rrow, stats = range_check(pair, [], [], 0, 1, 0, False, False, jt, [2], [1], f"edge {edge}")
            assert stats[2] == 1 and on[rrow[-1]] == edge
    finally:
        pair.free()


def test_the_cover_scan_takes_a_second_trip(gpu_ctx):
    """2^20 + 1 eligible right rows: the difference array has 2^20 + 2 entries, 1025 block sums, one more than a trip of the
    carry scan.  Three short intervals: at the front, ending on position 2^20 (the first entry of the second trip), and the last
    position alone."""
    rng = np.random.default_rng(85)
    nr = (1 << 20) + 1
    on = rng.permutation(nr)
    pair = simple_pair(gpu_ctx, [0, nr - 4, nr - 1], [2, nr - 2, nr - 1], on)
    try:
        _, rrow, stats = range_check(pair, [], [], 0, 1, 0, False, False, RIGHT, [2], [1], "2^20 + 1 right rows")
        assert stats == [RANGE_JOIN, 7, nr - 7, 7]
        covered = np.isin(on, [0, 1, 2, nr - 4, nr - 3, nr - 2, nr - 1])
        assert np.array_equal(rrow[7:], np.nonzero(~covered)[0])
    finally:
        pair.free()


@pytest.mark.parametrize("empty", ["left", "right", "both"])
def test_range_empty_sides(gpu_ctx, empty):
    rng = np.random.default_rng(86)
    nl, nr = (0 if empty in ("left", "both") else 50), (0 if empty in ("right", "both") else 70)
    lcols = [Column(I32, rng.integers(0, 3, nl).astype(np.int32))] + bounds(D, rng, nl, 12, 0.0) + range_payload(rng, nl)
    rcols = [Column(I32, rng.integers(0, 3, nr).astype(np.int32)), value_column(D, rng, nr, 12, 0.0)] + range_payload(rng, nr)
    pair = Pair(gpu_ctx, lcols, rcols)
    try:
        for jt in OUTER:
            _, _, stats = range_check(pair, [0], [0], 1, 2, 1, False, False, jt, [3, 4], [2, 3], f"empty {empty}")
            assert stats[1:] == [nl if jt == FULL and nr == 0 else 0, nr, 0]
    finally:
        pair.free()


def test_the_same_bytes_on_every_run_and_context_range(gpu_ctx):
    rng = np.random.default_rng(87)
    nl, nr = 5003, 3001
    lcols = [Column(I32, rng.integers(0, 9, nl).astype(np.int32))] + bounds(I64, rng, nl, 60, 0.05, 8) + range_payload(rng, nl)
    rcols = [Column(I32, rng.integers(0, 9, nr).astype(np.int32)), value_column(I64, rng, nr, 60, 0.05)] + range_payload(rng, nr)

    def run(ctx):
        pair = Pair(ctx, lcols, rcols)
        out = ctx.range_join(pair.lres, pair.rres, [0], [0], 1, 2, 1, False, True, FULL, [3, 4], [2, 3])
        raw = column_bytes(out)
        out.free()
        pair.free()
        return raw

    first = run(gpu_ctx)
    assert len(first[0][0]) > 8 * nl and run(gpu_ctx) == first
    other = E.Context(device=0)
    try:
        assert run(other) == first
    finally:
        other.close()
