"""The hash equi-join on the device (qe_join_build / qe_join_probe / qe_batch_from_result).

The expectation is always the host branch of ``HashJoinOperator`` over the same columns (a dict from the key tuple to the
list of build rows, probe side outside).  Every probe side and every build side carries an INT64 row id; the two row-id
output columns are compared exactly, which pins the pairing AND the order.  Every output column is then compared in full
-- type, dictionary, validity, value, the zeroed value under a LEFT "none" -- with join_reference.expected_columns over
the host branch's pairs, and a handful of rows (first, last, a few in between) once more through boxed values.  Keys come
from the special-value pools of test_gpu_order_by_keys.py."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import Fn, assert_columns_equal, col, fn, num
from join_reference import assert_join_output, expected_columns, expected_nullable, reference_pairs
from test_gpu_order_by_keys import DOUBLES, INT64S, STRINGS, Rows, make_key
from queryengine_amd import AggregationFunction as AF
from queryengine_amd import Column, ColumnarTable, ColumnExpression, DataType, Field, Schema
from queryengine_amd import engine as E
from queryengine_amd import native as N
from queryengine_amd.operators import (ColumnarScanOperator, GpuFilterProjectOperator, HashJoinOperator, OrderByOperator,
                                       map as op_map)

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
INNER, LEFT, SEMI, ANTI = N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI
JOIN_NAMES = {INNER: "INNER", LEFT: "LEFT", SEMI: "SEMI", ANTI: "ANTI"}
INVALID_ARG = 1
TAGS = ["t0", "", "täg", "t3"]
SIZES = [(0, 5), (5, 0), (1, 1), (63, 64), (65, 129), (4099, 1031)]
# which kind each side is, per size: every kind appears on every side
KINDS = [("batch", "result"), ("result", "batch"), ("result", "result"), ("batch", "batch"), ("batch", "result"), ("result", "batch")]


def payload(rng, n, with_tag):
    """(INT64 row id, nullable BOOLEAN flag[, nullable STRING tag, DOUBLE value without validity])."""
    cols = [Column(I64, np.arange(n, dtype=np.int64)), Column(B, rng.random(n) > 0.3, (rng.random(n) > 0.2) if n else None)]
    if with_tag:
        cols.append(Column(S, rng.integers(0, len(TAGS), n).astype(np.int32), (rng.random(n) > 0.1) if n else None, TAGS))
        cols.append(Column(D, rng.integers(-50, 50, n).astype(np.float64)))
    return cols


def as_side(ctx, cols, kind):
    """The columns as a join side: a pinned batch, or the result of an identity projection over it.  -> (side, to free)"""
    batch = E.DeviceBatch.from_columns(ctx, cols)
    if kind == "batch":
        return batch, [batch]
    res = E.filter_project(ctx, batch, None, [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)])
    return res, [res, batch]


def boxed(cols, only=None):
    n = len(cols[0])
    keep = range(len(cols)) if only is None else only
    lists = {c: cols[c].to_list() for c in keep}
    return [[lists[c][i] if c in lists else None for c in range(len(cols))] for i in range(n)]


def host_pairs(pcols, bcols, pk, bk, jt):
    """[(probe row id, build row id | None)] of the host branch; the row ids stand behind the key columns of each side."""
    prid, brid = len(pk), len(bk)
    pairs = jt in (INNER, LEFT)
    op = HashJoinOperator(Rows(boxed(pcols, list(pk) + [prid])), Rows(boxed(bcols, list(bk) + [brid])), pk, bk, jt, [prid], [brid] if pairs else None)
    return [(r[0], r[1] if pairs else None) for r in op_map(op, lambda r: list(r))]


def same(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return (a != a and b != b) or (a == b and math.copysign(1.0, a) == math.copysign(1.0, b))
    return type(a) is type(b) and a == b


def side_nullable(side, cols):
    """Which columns of a join side carry a validity bitmap on the device."""
    if isinstance(side, E.Result):
        return [bool(side.view(c).nullable) for c in range(len(cols))]
    return [c.valid is not None for c in cols]


def check_result(res, want, pcols, bcols, probe_out, build_out, jt, what="", sides=None):
    """`res` against the pairs `want`: both row-id columns exactly, EVERY column in full against expected_columns, sample
    rows in every column through boxed values.  The row id of a side is found by its position in probe_out / build_out
    (the column index nkeys of the side).  `sides` = (probe side, build side) as given to the join: checks nullability too."""
    m = len(want)
    assert res.count == m, (what, res.count, m)
    out = res.to_columns()
    assert len(out) == len(probe_out) + len(build_out)
    prow = np.array([p for p, _ in want], dtype=np.int64)
    brow = np.array([-1 if b is None else b for _, b in want], dtype=np.int64) if jt in (INNER, LEFT) else np.zeros(0, dtype=np.int64)
    assert_join_output(out, expected_columns(pcols, bcols, prow, brow, probe_out, build_out, jt), brow if jt in (INNER, LEFT) else None,
                       len(probe_out), what)
    if sides is not None:
        nullable = expected_nullable(side_nullable(sides[0], pcols), side_nullable(sides[1], bcols), probe_out, build_out, jt)
        assert [bool(res.view(k).nullable) for k in range(len(out))] == nullable, what
    for k, c in enumerate(probe_out):
        src = pcols[c]
        assert out[k].type == src.type
        if src.type == S:
            assert out[k].dictionary == src.dictionary
        if src.type == I64 and src.valid is None and np.array_equal(src.data, np.arange(len(src))):   # the row id
            assert out[k].valid is None
            assert np.array_equal(out[k].data, np.array([p for p, _ in want], dtype=np.int64)), what
    for k, c in enumerate(build_out):
        g, src = out[len(probe_out) + k], bcols[c]
        assert g.type == src.type
        if src.type == S:
            assert g.dictionary == src.dictionary
        if src.type == I64 and src.valid is None and np.array_equal(src.data, np.arange(len(src))):
            have = np.array([b is not None for _, b in want], dtype=bool)
            gv = g.valid if g.valid is not None else np.ones(m, dtype=bool)
            assert np.array_equal(gv, have), what
            assert np.array_equal(g.data[have], np.array([b for _, b in want if b is not None], dtype=np.int64)), what
    for j in sorted({0, 1, m // 3, m // 2, (2 * m) // 3, m - 2, m - 1} & set(range(m))):
        p, b = want[j]
        for k, c in enumerate(probe_out):
            assert same(out[k].value(j), pcols[c].value(p)), (what, j, k)
        for k, c in enumerate(build_out):
            assert same(out[len(probe_out) + k].value(j), None if b is None else bcols[c].value(b)), (what, j, k)
    return out


def run_case(ctx, pcols, bcols, pk, bk, jt, kinds=("batch", "batch"), what=""):
    """Build + probe with every payload column in the output, compared with the host branch."""
    pairs = jt in (INNER, LEFT)
    probe_out = list(range(len(pk), len(pcols))) + [pk[0]]
    build_out = (list(range(len(bk), len(bcols))) + [bk[0]]) if pairs else []
    want = host_pairs(pcols, bcols, pk, bk, jt)
    prow, brow = reference_pairs(pcols, bcols, pk, bk, jt)                       # the numpy reference agrees on every case here
    assert prow.tolist() == [p for p, _ in want] and (not pairs or [None if b < 0 else b for b in brow.tolist()] == [b for _, b in want])
    pside, pfree = as_side(ctx, pcols, kinds[0])
    bside, bfree = as_side(ctx, bcols, kinds[1])
    table = ctx.join_build(bside, bk)
    try:
        keyed = np.ones(len(bcols[0]), dtype=bool)
        for c in bk:
            if bcols[c].valid is not None:
                keyed &= bcols[c].valid
        assert table.rows == int(keyed.sum())
        res = table.probe(pside, pk, jt, probe_out, build_out)
        try:
            check_result(res, want, pcols, bcols, probe_out, build_out, jt, what, (pside, bside))
            st = ctx.last_join_stats()
            assert st[:3] == [table.rows, len(pcols[0]), len(want)], st
        finally:
            res.free()
    finally:
        table.free()
        for h in pfree + bfree:
            h.free()
    return want


@pytest.mark.parametrize("t", [D, I64, I32, S, B], ids=lambda t: t.name)
@pytest.mark.parametrize("jt", [INNER, LEFT, SEMI, ANTI], ids=lambda j: JOIN_NAMES[j])
def test_every_join_type_and_key_type(gpu_ctx, jt, t):
    matched = 0
    for (np_, nb), kinds in zip(SIZES, KINDS):
        rng = np.random.default_rng(1000 * jt + 10 * int(t) + np_)
        pcols = [make_key(t, rng, np_, coarse=True)] + payload(rng, np_, False)
        bcols = [make_key(t, rng, nb, coarse=True)] + payload(rng, nb, True)
        want = run_case(gpu_ctx, pcols, bcols, [0], [0], jt, kinds, f"{JOIN_NAMES[jt]} {t.name} {np_}x{nb}")
        matched += len(want)
    assert matched > 0


def test_string_keys_with_different_dictionaries(gpu_ctx):
    rng = np.random.default_rng(31)
    pdict = ["x", "b", "a", "q", "～", "aa", "\U0001F600"]                     # "x", "q" only here
    bdict = ["aa", "a", "zz", "b", "\U0001F600", "～", "a", "Zü"]               # "zz", "Zü" only here; "a" listed twice
    np_, nb = 1500, 333
    pcols = [Column(S, rng.integers(0, len(pdict), np_).astype(np.int32), rng.random(np_) > 0.05, pdict)] + payload(rng, np_, False)
    bcols = [Column(S, rng.integers(0, len(bdict), nb).astype(np.int32), rng.random(nb) > 0.05, bdict)] + payload(rng, nb, True)
    for jt in (INNER, LEFT, SEMI, ANTI):
        want = run_case(gpu_ctx, pcols, bcols, [0], [0], jt, ("result", "batch"), JOIN_NAMES[jt])
        if jt == INNER:   # both spellings of "a" on the build side match a probe "a"
            codes = {int(bcols[0].data[b]) for p, b in want if pcols[0].value(p) == "a"}
            assert codes == {1, 6}
        if jt == ANTI:
            assert {pcols[0].value(p) for p, _ in want} >= {"x", "q", None}


def mixed_keys(rng, n, types):
    return [make_key(t, rng, n, coarse=True, null_share=0.05) for t in types]


@pytest.mark.parametrize("types", [(I32, S), (B, I64, D, S)], ids=["two", "four"])
def test_keys_of_several_columns_with_mixed_types(gpu_ctx, types):
    rng = np.random.default_rng(32 + len(types))
    np_, nb = 3001, 2049
    k = len(types)
    # few distinct values per column so that whole tuples meet: the pools are cut down to their first entries
    def cut(c):
        if c.type == S:
            return Column(S, c.data % 3, c.valid, c.dictionary)
        if c.type == D:
            return Column(D, np.where(np.isin(c.data, DOUBLES[:2]) | np.isnan(c.data), c.data, 1.5), c.valid)   # 0.0, -0.0, NaN, 1.5
        if c.type == I64:
            return Column(I64, np.where(np.isin(c.data, INT64S[3:5]), c.data, 0), c.valid)                        # max, min, 0
        if c.type == I32:
            return Column(I32, c.data % 4, c.valid)
        return c
    pcols = [cut(c) for c in mixed_keys(rng, np_, types)] + payload(rng, np_, False)
    bcols = [cut(c) for c in mixed_keys(rng, nb, types)] + payload(rng, nb, True)
    keys = list(range(k))
    for jt in (INNER, LEFT, SEMI, ANTI):
        want = run_case(gpu_ctx, pcols, bcols, keys, keys, jt, ("batch", "result"), JOIN_NAMES[jt])
        if jt == INNER:
            assert len(want) > np_
            for p, b in want[:: max(1, len(want) // 50)]:      # a row with a NULL in one key column never appears
                assert all(pcols[c].value(p) is not None and bcols[c].value(b) is not None for c in keys)
    # the key columns pair by position: build side with its key columns in another order
    order = keys[::-1]
    bswapped = [bcols[c] for c in order] + bcols[k:]
    run_case(gpu_ctx, pcols, bswapped, keys, [order.index(c) for c in keys], INNER, ("batch", "batch"), "swapped")


def test_expansion(gpu_ctx):
    rng = np.random.default_rng(34)
    # 3000 probe rows all match ONE build row
    pcols = [Column(I64, np.full(3000, 3, dtype=np.int64))] + payload(rng, 3000, False)
    bcols = [Column(I64, np.arange(5, dtype=np.int64))] + payload(rng, 5, True)
    want = run_case(gpu_ctx, pcols, bcols, [0], [0], INNER)
    assert want == [(i, 3) for i in range(3000)]
    # 1 probe row matches 20 000 build rows (every second one), in build-row order
    pcols = [Column(I32, np.array([7], dtype=np.int32))] + payload(rng, 1, False)
    bcols = [Column(I32, np.tile(np.array([7, 8], dtype=np.int32), 20_000))] + payload(rng, 40_000, True)
    want = run_case(gpu_ctx, pcols, bcols, [0], [0], INNER)
    assert want == [(0, 2 * i) for i in range(20_000)]
    # 50 x 400 rows of one key among others
    pk = np.where(np.arange(500) % 10 == 0, 1.5, np.arange(500) + 100.0)
    bk = np.where(np.arange(2000) % 5 == 0, 1.5, -np.arange(2000) - 1.0)
    pcols = [Column(D, pk)] + payload(rng, 500, False)
    bcols = [Column(D, bk)] + payload(rng, 2000, True)
    for jt in (INNER, LEFT):
        want = run_case(gpu_ctx, pcols, bcols, [0], [0], jt)
        assert len(want) == 20_000 + (450 if jt == LEFT else 0)
        first = [b for p, b in want if p == 0]
        assert first == list(range(0, 2000, 5))          # the matches of one probe row in build-row order


@pytest.mark.parametrize("nkeys", [1, 2])
def test_keys_that_share_a_hash_are_told_apart_by_the_key(gpu_ctx, monkeypatch, nkeys):
    """QE_JOIN_HASH_BITS=3 (read when a table is built) leaves 8 distinct hashes for 2000 distinct keys."""
    rng = np.random.default_rng(35)
    n = 2000
    keys = rng.permutation(n).astype(np.int64) * 7919 - 5_000_000
    bkeys = [Column(I64, keys)] + ([Column(I32, (keys % 13).astype(np.int32))] if nkeys == 2 else [])
    sel = rng.integers(0, n + 200, 3000)                                          # some probe keys exist nowhere
    pk = np.where(sel < n, keys[np.minimum(sel, n - 1)], 10 ** 12 + sel)
    pkeys = [Column(I64, pk)] + ([Column(I32, (pk % 13).astype(np.int32))] if nkeys == 2 else [])
    pcols, bcols = pkeys + payload(rng, 3000, False), bkeys + payload(rng, n, True)
    kc = list(range(nkeys))
    plain = run_case(gpu_ctx, pcols, bcols, kc, kc, LEFT)
    plain_run = gpu_ctx.last_join_stats()[3]
    monkeypatch.setenv("QE_JOIN_HASH_BITS", "3")
    for jt in (LEFT, INNER, SEMI, ANTI):
        shared = run_case(gpu_ctx, pcols, bcols, kc, kc, jt)
        run = gpu_ctx.last_join_stats()[3]
        assert run > 1 and run >= n // 8 and run > plain_run, (run, plain_run)   # the switch took effect
        if jt == LEFT:
            assert shared == plain


def test_left_join_nulls_every_build_column(gpu_ctx):
    rng = np.random.default_rng(36)
    np_, nb = 777, 100
    pcols = [Column(I32, rng.integers(0, 200, np_).astype(np.int32))] + payload(rng, np_, False)
    bcols = [Column(I32, rng.permutation(200)[:nb].astype(np.int32))] + payload(rng, nb, True)
    assert bcols[4].valid is None and bcols[1].valid is None                    # row id and value: no validity on the build side
    pside, pfree = as_side(gpu_ctx, pcols, "batch")
    bside, bfree = as_side(gpu_ctx, bcols, "batch")
    table = gpu_ctx.join_build(bside, [0])
    res = table.probe(pside, [0], LEFT, [1], [0, 1, 2, 3, 4])
    want = host_pairs(pcols, bcols, [0], [0], LEFT)
    out = check_result(res, want, pcols, bcols, [1], [0, 1, 2, 3, 4], LEFT)
    unmatched = np.array([b is None for _, b in want])
    assert 0 < unmatched.sum() < len(want)
    for k in range(1, 6):                                                        # INT32 key, row id, BOOLEAN, STRING, DOUBLE
        assert res.view(k).nullable == 1 and res.view(k).validity
        assert out[k].valid is not None and not out[k].valid[unmatched].any()
        if out[k].type != B:
            assert not out[k].data[unmatched].any()                              # a "none" row gives a zeroed value
    assert res.view(0).nullable == 0
    inner = table.probe(pside, [0], INNER, [1], [1, 4])
    assert inner.view(1).nullable == 0 and inner.view(2).nullable == 0          # INNER: nullability is the source's
    for h in [inner, res, table] + pfree + bfree:
        h.free()


def test_left_join_without_a_match_at_the_word_boundaries(gpu_ctx):
    """65 probe rows, every matched one with exactly one partner, rows 0, 63 and 64 without: the "no row" id stands at the
    first bit of a bitmap word, at its last bit and alone in the next word.  Build columns: a BOOLEAN without validity (all
    true), a nullable INT32 and a DOUBLE without validity -- its output bitmap comes from a null source bitmap, all ones
    except under "no row".  Every value beside a "no row" is nonzero / true / valid, so a zero there is the sentinel's."""
    rng = np.random.default_rng(38)
    n, nb, none = 65, 80, [0, 63, 64]
    pkey = rng.integers(0, nb, n).astype(np.int32)
    pkey[none] = [1000, 1001, 1002]
    pcols = [Column(I32, pkey), Column(I64, np.arange(n, dtype=np.int64))]
    ivalid = rng.random(nb) > 0.2
    ivalid[pkey[[1, 62]]] = True                                                 # the neighbours of the unmatched rows are valid
    bcols = [Column(I32, np.arange(nb, dtype=np.int32)), Column(B, np.ones(nb, dtype=bool)),
             Column(I32, rng.integers(1, 1000, nb).astype(np.int32), ivalid), Column(D, rng.integers(1, 50, nb).astype(np.float64))]
    probe_out, build_out = [1], [1, 2, 3]
    prow, brow = reference_pairs(pcols, bcols, [0], [0], LEFT)
    assert prow.tolist() == list(range(n)) and np.nonzero(brow < 0)[0].tolist() == none
    want = expected_columns(pcols, bcols, prow, brow, probe_out, build_out, LEFT)
    pside, pfree = as_side(gpu_ctx, pcols, "batch")
    bside, bfree = as_side(gpu_ctx, bcols, "batch")
    table = gpu_ctx.join_build(bside, [0])
    res = table.probe(pside, [0], LEFT, probe_out, build_out)
    try:
        assert res.count == n
        out = res.to_columns()
        assert_join_output(out, want, brow, len(probe_out), "LEFT, no match at rows 0, 63, 64")
        assert [bool(res.view(k).nullable) for k in range(res.ncols)] == [False, True, True, True]
        matched = brow >= 0
        for k in (1, 2, 3):
            assert not out[k].valid[none].any() and not out[k].data[none].any()
        assert out[1].valid[matched].all() and out[1].data[matched].all()         # BOOLEAN: bits of the neighbours untouched
        assert out[3].valid[matched].all() and (out[3].data[matched] > 0).all()   # DOUBLE: "all ones" from the null bitmap
        assert np.array_equal(out[2].valid[matched], ivalid[brow[matched]]) and out[2].valid[[1, 62]].all()
    finally:
        for h in [res, table] + pfree + bfree:
            h.free()


def test_empty_results_through_every_call_that_makes_one(gpu_ctx):
    """Zero rows through every call that builds a result: a concatenation of empty parts, ORDER BY with and without LIMIT, an
    INNER join whose probe side matches nothing, a LEFT join of no probe rows, the window operator and a hashed GROUP BY
    whose filter keeps no row.  Each gives the right column types and count 0, can be read and can be freed -- every
    buffer of such a result is a zero-byte request to the device pool."""
    ctx = gpu_ctx
    rng = np.random.default_rng(39)
    n = 100
    cols = [Column(I32, rng.integers(0, 10, n).astype(np.int32)), Column(D, rng.normal(0, 1, n), rng.random(n) > 0.2),
            Column(B, rng.random(n) > 0.5, rng.random(n) > 0.2), Column(S, rng.integers(0, len(TAGS), n).astype(np.int32), None, TAGS),
            Column(I64, np.arange(n, dtype=np.int64))]
    types = [c.type for c in cols]
    batch = E.DeviceBatch.from_columns(ctx, cols)
    ident = [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)]
    nothing = ctx.compile(fn(Fn.CMP_LT, col("id", 4, I64), num(-1.0)))
    full = E.filter_project(ctx, batch, None, ident)
    empty = E.filter_project(ctx, batch, nothing, ident)
    made = [full, empty]

    def check(res, want_types, what):
        made.append(res)
        assert res.count == 0 and res.ncols == len(want_types), what
        out = res.to_columns()
        assert [c.type for c in out] == want_types and all(len(c) == 0 for c in out), what
        for k, t in enumerate(want_types):
            assert res.view(k).type == int(t), what
            if t == S:
                assert out[k].dictionary == TAGS, what

    try:
        assert full.count == n and empty.count == 0
        check(ctx.concat([empty, empty, empty]), types, "concat of empty parts")
        check(ctx.order_by_keys(empty, [(0, False), (1, True)]), types, "ORDER BY over no rows")
        check(ctx.order_by_keys(empty, [(1, True)], limit=3), types, "ORDER BY .. LIMIT over no rows")
        check(ctx.order_by_keys(full, [(1, True)], limit=0), types, "ORDER BY .. LIMIT 0")
        table = ctx.join_build(full, [0])                                       # keys 0 .. 9
        made.append(table)
        other = E.DeviceBatch.from_columns(ctx, [Column(I32, np.arange(100, 150, dtype=np.int32)), Column(D, rng.normal(0, 1, 50))])
        made.append(other)
        check(table.probe(other, [0], INNER, [0, 1], [1, 2, 3, 4]), [I32, D, D, B, S, I64], "INNER join without a match")
        assert ctx.last_join_stats()[:3] == [n, 50, 0]
        check(table.probe(empty, [0], LEFT, [0, 4], [1, 2, 3]), [I32, I64, D, B, S], "LEFT join of no probe rows")
        check(ctx.window(empty, [0], [(4, False)], [(N.WIN_ROW_NUMBER, 0, 0), (N.WIN_SUM, 1, 0), (N.WIN_LAG, 3, 1)]),
              types + [I64, D, S], "window over no rows")
        keys, exprs = [ctx.compile(col("v", 1, D))], [ctx.compile(col("v", 1, D)), ctx.compile(col("v", 1, D))]
        check(E.filter_groupby(ctx, batch, nothing, keys, exprs, [int(AF.SUM), int(AF.COUNT)]), [D, D, D], "hashed GROUP BY, no row kept")
        assert ctx.last_form == N.FORM_GROUPBY_HASHED
    finally:
        for h in made[::-1] + [batch]:
            h.free()


def test_the_same_bytes_on_every_run_and_context(gpu_ctx):
    rng = np.random.default_rng(37)
    np_, nb = 8_009, 2_003
    pcols = [make_key(I64, rng, np_, coarse=False)] + payload(rng, np_, False)
    bcols = [make_key(I64, rng, nb, coarse=False)] + payload(rng, nb, True)

    def run(ctx):
        pside, pfree = as_side(ctx, pcols, "batch")
        bside, bfree = as_side(ctx, bcols, "batch")
        table = ctx.join_build(bside, [0])
        res = table.probe(pside, [0], LEFT, [0, 1, 2], [0, 1, 2, 3, 4])
        raw = []
        for c in res.to_columns():
            raw.append((c.data.tobytes(), None if c.valid is None else c.valid.tobytes()))
        for h in [res, table] + pfree + bfree:
            h.free()
        return raw

    first = run(gpu_ctx)
    assert len(first[0][0]) > 8 * np_
    assert run(gpu_ctx) == first
    other = E.Context(device=0)
    try:
        assert run(other) == first
    finally:
        other.close()


def test_one_table_probed_twice(gpu_ctx):
    rng = np.random.default_rng(38)
    nb = 700
    bcols = [make_key(D, rng, nb, coarse=True)] + payload(rng, nb, True)
    bside, bfree = as_side(gpu_ctx, bcols, "result")
    table = gpu_ctx.join_build(bside, [0])
    keyed = int(bcols[0].valid.sum())
    assert table.rows == keyed < nb
    for seed, n, jt, kind in ((1, 900, INNER, "batch"), (2, 257, ANTI, "result"), (3, 900, LEFT, "result")):
        r = np.random.default_rng(seed)
        pcols = [make_key(D, r, n, coarse=True)] + payload(r, n, False)
        pside, pfree = as_side(gpu_ctx, pcols, kind)
        pairs = jt in (INNER, LEFT)
        probe_out, build_out = [1, 2, 0], ([1, 2, 3, 4, 0] if pairs else [])
        res = table.probe(pside, [0], jt, probe_out, build_out)
        check_result(res, host_pairs(pcols, bcols, [0], [0], jt), pcols, bcols, probe_out, build_out, jt)
        for h in [res] + pfree:
            h.free()
        assert table.rows == keyed                                               # still usable
    table.free()
    for h in bfree:
        h.free()


def joined_host_columns(pcols, bcols, want, probe_out, build_out):
    """The host-joined rows as ordinary columns (to pin as an ordinary batch)."""
    cols = []
    for c in probe_out:
        cols.append(Column.from_values(pcols[c].type, [pcols[c].value(p) for p, _ in want], pcols[c].dictionary))
    for c in build_out:
        cols.append(Column.from_values(bcols[c].type, [None if b is None else bcols[c].value(b) for _, b in want], bcols[c].dictionary))
    return cols


def test_a_join_result_feeds_the_next_plan(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(39)
    np_, nb = 6000, 300
    pcols = [Column(I32, rng.integers(0, 400, np_).astype(np.int32))] + payload(rng, np_, False) + [Column(D, rng.integers(-9, 9, np_).astype(np.float64))]
    bcols = [Column(I32, rng.permutation(400)[:nb].astype(np.int32))] + payload(rng, nb, True)
    pside, pfree = as_side(ctx, pcols, "batch")
    bside, bfree = as_side(ctx, bcols, "result")
    table = ctx.join_build(bside, [0])
    probe_out, build_out = [1, 3], [3, 4, 1]           # probe row id, probe value | build tag, build value, build row id
    for jt in (INNER, LEFT):
        joined = table.probe(pside, [0], jt, probe_out, build_out)
        want = host_pairs(pcols, bcols, [0], [0], jt)
        check_result(joined, want, pcols, bcols, probe_out, build_out, jt)
        hcols = joined_host_columns(pcols, bcols, want, probe_out, build_out)
        hbatch = E.DeviceBatch.from_columns(ctx, hcols)
        jbatch = joined.as_batch()
        assert jbatch.nrows == joined.count == len(want) and jbatch.ncols == 5
        assert [jbatch.column_type(i) for i in range(5)] == [c.type for c in hcols]
        # GROUP BY a build column, SUM of a probe column (integer valued: exact in any order)
        tag, val, bval = col("tag", 2, S), col("v", 1, D), col("bv", 3, D)
        keys, exprs, aggs = [ctx.compile(tag)], [ctx.compile(val), ctx.compile(bval)], [int(AF.SUM), int(AF.COUNT)]
        got, exp = E.filter_groupby(ctx, jbatch, None, keys, exprs, aggs), E.filter_groupby(ctx, hbatch, None, keys, exprs, aggs)
        assert got.count == exp.count > 1
        for g, w in zip(got.to_columns(), exp.to_columns()):
            assert_columns_equal(g, w, "group by over the join")
        got.free(); exp.free()
        # a filter (HAVING-like) and a projection
        flt = ctx.compile(fn(Fn.CMP_GT, val, num(2.0)))
        projs = [ctx.compile(col("rid", 0, I64)), ctx.compile(fn(Fn.ADD, val, bval)), ctx.compile(tag)]
        got, exp = E.filter_project(ctx, jbatch, flt, projs), E.filter_project(ctx, hbatch, flt, projs)
        assert 0 < got.count == exp.count < len(want)
        for g, w in zip(got.to_columns(), exp.to_columns()):
            assert_columns_equal(g, w, "filter + projection over the join")
        got.free(); exp.free()
        vals, nsel = E.filter_aggregate(ctx, jbatch, flt, [ctx.compile(val)], [int(AF.SUM)])
        evals, ensel = E.filter_aggregate(ctx, hbatch, flt, [ctx.compile(val)], [int(AF.SUM)])
        assert (vals, nsel) == (evals, ensel)
        # ORDER BY .. LIMIT directly on the join result
        srt = ctx.order_by_keys(joined, [(1, True), (4, False)], 40)
        rows = boxed(hcols)
        exp_rows = op_map(OrderByOperator(Rows(rows), 1, [(1, True), (4, False)], 40), lambda r: list(r))
        got_rows = boxed(srt.to_columns())
        assert len(got_rows) == 40 and all(same(a, b) for gr, er in zip(got_rows, exp_rows) for a, b in zip(gr, er))
        srt.free()
        jbatch.free(); hbatch.free(); joined.free()
    # a zero-row result as a batch
    nothing = [Column(I32, np.full(10, -1, dtype=np.int32))] + payload(rng, 10, False) + [Column(D, np.zeros(10))]
    nside, nfree = as_side(ctx, nothing, "batch")
    empty = table.probe(nside, [0], INNER, probe_out, build_out)
    assert empty.count == 0
    ebatch = empty.as_batch()
    assert ebatch.nrows == 0 and ebatch.ncols == 5
    res = E.filter_project(ctx, ebatch, None, [ctx.compile(col("v", 1, D))])
    assert res.count == 0
    for h in [res, ebatch, empty, table] + nfree + pfree + bfree:
        h.free()


def test_invalid_arguments_leave_the_context_usable(gpu_ctx, native_lib):
    lib, ctx = native_lib, gpu_ctx
    rng = np.random.default_rng(40)
    pcols = [Column(I64, rng.integers(0, 50, 300)), Column(I32, rng.integers(0, 50, 300).astype(np.int32))] + payload(rng, 300, False)
    bcols = [Column(I64, rng.integers(0, 50, 100)), Column(I32, rng.integers(0, 50, 100).astype(np.int32))] + payload(rng, 100, True)
    pside, pfree = as_side(ctx, pcols, "batch")
    bside, bfree = as_side(ctx, bcols, "result")
    table = ctx.join_build(bside, [0])
    pin, bin_ = N.JoinInput(None, pside.handle), N.JoinInput(bside.handle, None)

    def arr(v):
        return (C.c_int32 * 8)(*v)

    def build(keys, nkeys):
        out = C.c_void_p(0xdead)
        st = lib.qe_join_build(ctx.handle, C.byref(bin_), arr(keys), nkeys, C.byref(out))
        assert out.value is None
        return st

    def probe(keys, nkeys, jt, pout, bout, tab=table.handle):
        out = C.c_void_p(0xdead)
        st = lib.qe_join_probe(ctx.handle, tab, C.byref(pin), arr(keys), nkeys, jt, arr(pout), len(pout), arr(bout), len(bout), C.byref(out))
        assert out.value is None
        return st

    assert build([0], 0) == INVALID_ARG
    assert build([0, 1, 0, 1, 0], 5) == INVALID_ARG
    assert build([9], 1) == INVALID_ARG
    assert build([-1], 1) == INVALID_ARG
    assert probe([1], 1, INNER, [2], [2]) == INVALID_ARG                         # INT32 against the table's INT64 key
    assert b"INT32" in lib.qe_last_error(ctx.handle) or b"int32" in lib.qe_last_error(ctx.handle).lower()
    assert probe([0], 0, INNER, [2], [2]) == INVALID_ARG
    assert probe([0, 1, 0, 1, 0], 5, INNER, [2], [2]) == INVALID_ARG
    assert probe([0, 1], 2, INNER, [2], [2]) == INVALID_ARG                      # not the table's number of keys
    assert probe([7], 1, INNER, [2], [2]) == INVALID_ARG
    assert probe([0], 1, INNER, [4], [2]) == INVALID_ARG                         # probe side has columns 0..3
    assert probe([0], 1, INNER, [2], [6]) == INVALID_ARG                         # build side has columns 0..5
    assert probe([0], 1, SEMI, [2], [2]) == INVALID_ARG                          # build columns with SEMI
    assert probe([0], 1, ANTI, [2], [2]) == INVALID_ARG
    assert probe([0], 1, 4, [2], [2]) == INVALID_ARG
    assert probe([0], 1, INNER, [], []) == INVALID_ARG                           # no output column
    assert probe([0], 1, INNER, [2], [2], tab=None) == INVALID_ARG
    table.free()
    for h in pfree + bfree:
        h.free()
    run_case(ctx, pcols, bcols, [0, 1], [0, 1], INNER, ("batch", "result"))      # the context still works


def test_hash_join_operator_on_gpu_sources(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(41)
    nf, nd = 5000, 64
    names = ["DE", "AT", "CH", "FR"]
    fact = ColumnarTable(Schema([Field("k", I32), Field("x", D), Field("id", I64)]),
                         [Column(I32, rng.integers(0, 80, nf).astype(np.int32), rng.random(nf) > 0.03), Column(D, rng.random(nf)),
                          Column(I64, np.arange(nf, dtype=np.int64))])
    dim = ColumnarTable(Schema([Field("k", I32), Field("c", S)]),
                        [Column(I32, np.arange(nd, dtype=np.int32)), Column(S, rng.integers(0, 4, nd).astype(np.int32), rng.random(nd) > 0.1, names)])

    def sources():
        probe = GpuFilterProjectOperator(ctx, ColumnarScanOperator(fact, ["k", "x", "id"]), fn(Fn.CMP_LT, col("x", 1, D), num(0.5)),
                                         [col("k", 0, I32), col("x", 1, D), col("id", 2, I64)])
        build = GpuFilterProjectOperator(ctx, ColumnarScanOperator(dim, ["k", "c"]), None, [col("k", 0, I32), col("c", 1, S)])
        return probe, build

    for jt in (INNER, LEFT, SEMI, ANTI):
        pairs = jt in (INNER, LEFT)
        probe, build = sources()
        dev = HashJoinOperator(probe, build, [0], [0], jt, [2, 1], [1] if pairs else None)
        assert dev._on_device and dev.ctx is ctx
        host = HashJoinOperator(Rows(op_map(probe, lambda r: list(r))), Rows(op_map(build, lambda r: list(r))), [0], [0], jt, [2, 1],
                                [1] if pairs else None)
        assert not host._on_device
        got, want = op_map(dev, lambda r: list(r)), op_map(host, lambda r: list(r))
        assert len(got) == len(want) > 0 and got == want, JOIN_NAMES[jt]
    # an OrderByOperator on top sorts the join's result in HBM
    probe, build = sources()
    rows_host = op_map(HashJoinOperator(Rows(op_map(probe, lambda r: list(r))), Rows(op_map(build, lambda r: list(r))), [0], [0], LEFT, [2, 1], [1]),
                       lambda r: list(r))
    want = op_map(OrderByOperator(Rows(rows_host), 0, [(2, False), (1, True)], 100), lambda r: list(r))
    ctx.order_by_keys(E.filter_project(ctx, E.DeviceBatch.from_columns(ctx, [Column(I64, np.arange(3, dtype=np.int64))]), None,
                                       [ctx.compile(col("a", 0, I64))]), [(0, False)])       # leaves other sort stats behind
    before = ctx.last_sort_stats()
    got = op_map(OrderByOperator(HashJoinOperator(probe, build, [0], [0], LEFT, [2, 1], [1]), 0, [(2, False), (1, True)], 100), lambda r: list(r))
    assert got == want and len(got) == 100
    after = ctx.last_sort_stats()
    assert after != before and after["sorted_rows"] >= 100


def test_a_result_freed_before_its_batch_stays_readable(gpu_ctx):
    """qe_result_free while a batch of qe_batch_from_result is alive is deferred to the batch's qe_batch_free: the pool must
    not hand the buffers to the next result meanwhile."""
    ctx = gpu_ctx
    n = 10_000
    cols = [Column(I64, np.arange(n, dtype=np.int64)), Column(D, np.arange(n, dtype=np.float64) * 0.5)]
    projs = [ctx.compile(col("a", 0, I64)), ctx.compile(col("b", 1, D))]
    src = E.DeviceBatch.from_columns(ctx, cols)
    res = E.filter_project(ctx, src, None, projs)
    view = res.as_batch()
    res.free()                                               # before the batch
    other = E.DeviceBatch.from_columns(ctx, [Column(I64, np.full(n, -7, dtype=np.int64)), Column(D, np.full(n, -7.0))])
    clobber = E.filter_project(ctx, other, None, projs)      # same sizes: would take the freed buffers from the pool
    again = E.filter_project(ctx, view, None, projs)
    for g, w in zip(again.to_columns(), cols):
        assert_columns_equal(g, w, "view of a freed result")
    for h in (again, clobber, other, view, src):
        h.free()
