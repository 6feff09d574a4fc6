"""qe_result_set_op on the device: UNION, INTERSECT, EXCEPT, each with ALL.

The expectation is tests/setop_reference.py (numpy; proved equal to the host branch of ``SetOperator`` in
tests/test_setop_cpu.py).  Every output column is compared in full -- type, nullability, dictionary, validity, values by bits
(any NaN for any NaN) -- with no tolerance; counts and last_set_stats are checked too.  The value under a NULL is the source
row's and is not compared.  Sizes are those where the code changes path: word (64) and tile (2048) edges of the bitmaps, a right
side that lands at an unaligned bit offset, and more rows than one sweep of the two bitmap kernels (native.SETOP_BLOCKS).

Not tested: 2^32 - 1 rows or more; the planning-only error (a planning-only context cannot hold a result); a STRING column
without a dictionary, which cannot be built through the ABI; a result of zero columns, which no operator of the suite makes."""
import ctypes as C

import numpy as np
import pytest

from queryengine_amd import AggregationFunction as AF
from queryengine_amd import Column, ColumnExpression, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N

from setop_reference import Analysis, setop_reference
from window_reference import T, assert_window_output

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
U, I, X = N.SET_UNION, N.SET_INTERSECT, N.SET_EXCEPT
FORMS = [(op, all_) for op in (U, I, X) for all_ in (False, True)]
NAMES = {U: "UNION", I: "INTERSECT", X: "EXCEPT"}
INVALID_ARG, UNSUPPORTED = 1, 5
NAN, INF = float("nan"), float("inf")
STRINGS = ["b", "a", "", "B", "～", "\U0001F600", "aa", "Zü", "zz", "a "]     # not in sorted order
SEAM_LENGTHS = [1, 2, 63, 64, 65, 512, 513, 2048, 2049]
SWEEP = N.SETOP_BLOCKS * 256    # rows of one sweep of setop_side_bits / setop_keep


def build(ctx, cols):
    """filter_project over an identity projection: a result that holds exactly `cols`."""
    batch = E.DeviceBatch.from_columns(ctx, cols)
    projs = [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)]
    return batch, E.filter_project(ctx, batch, None, projs)


def nullable_of(res):
    return [bool(res.view(c).nullable) for c in range(res.ncols)]


def column_bytes(result):
    return [(c.data.tobytes(), None if c.valid is None else c.valid.tobytes()) for c in result.to_columns()]


def check_form(ctx, lcols, rcols, lres, rres, op, all_, what, analysis=None):
    """One qe_result_set_op against the reference; returns the expected columns."""
    what = f"{what}: {NAMES[op]}{' ALL' if all_ else ''}"
    want, stats = setop_reference(lcols, rcols, nullable_of(lres), nullable_of(rres), op, all_, analysis=analysis)
    out = ctx.set_op(lres, rres, op, all_)
    try:
        assert out.count == len(want[0].data), (what, out.count, len(want[0].data))
        assert ctx.last_set_stats() == stats, (what, ctx.last_set_stats(), stats)
        assert_window_output(out, want, what)
    finally:
        out.free()
    return want


def check_all_forms(ctx, lcols, rcols, what):
    lbatch, lres = build(ctx, lcols)
    rbatch, rres = build(ctx, rcols)
    shared = Analysis(lcols, rcols)           # the reference's sort, once for the six forms
    try:
        return {form: check_form(ctx, lcols, rcols, lres, rres, form[0], form[1], what, shared) for form in FORMS}
    finally:
        lres.free(); rres.free(); lbatch.free(); rbatch.free()


def tuple_columns(types, ids, rng, nullable=True, dictionary=STRINGS):
    """Columns whose row i is a function of ids[i] alone, validity included, so that equal ids are equal tuples: an INT64 or
    DOUBLE column is one-to-one in the id, the other types fold it.  The value under a NULL is random."""
    cols = []
    for k, t in enumerate(types):
        v = ids + 3 * k
        valid = (v % 5 != 1) if nullable else None
        if t == I64:
            data = (ids * 3 - 50).astype(np.int64)
        elif t == D:
            data = ids / 4.0 - 3.0 if k == 0 else np.array([NAN, -0.0, 0.0, INF, 1.5, -2.25])[v % 6]
        elif t == I32:
            data = (v % 7 - 3).astype(np.int32)
        elif t == B:
            data = (v % 3 == 0)
        else:
            data = (v % len(dictionary)).astype(np.int32)
        if valid is not None:
            noise = rng.integers(0, 2, len(ids))
            data = np.where(valid, data, (noise if t != S else noise % len(dictionary)).astype(data.dtype))
        cols.append(Column(t, data, valid, dictionary if t == S else None))
    return cols


def run_ids(rng, n, first_id):
    """n tuple ids in runs of the seam lengths (the last run cut), shuffled."""
    lengths = []
    while sum(lengths) < n:
        lengths.append(SEAM_LENGTHS[rng.integers(0, len(SEAM_LENGTHS))])
    ids = np.repeat(np.arange(len(lengths)) + first_id, lengths)[:n]
    return ids[rng.permutation(n)].astype(np.int64)


# ---- 1. word and tile seams --------------------------------------------------------------------------------------------------
SEAM_TYPES = [[I64, D, B, S], [D, I32, S, B], [I64, I32, B, D], [D, S, I32, I64]]


@pytest.mark.parametrize("aligned", [True, False], ids=["n-multiple-of-64", "n-ragged"])
@pytest.mark.parametrize("case, nl", list(enumerate([63, 64, 65, 3 * T + 37])))
def test_word_and_tile_seams(gpu_ctx, case, nl, aligned):
    rng = np.random.default_rng(500 + 2 * case + aligned)
    nr = 2 * T + (-nl) % 64 + (0 if aligned else 5)
    assert ((nl + nr) % 64 == 0) == aligned
    types = SEAM_TYPES[case]
    lids, rids = run_ids(rng, nl, 0), run_ids(rng, nr, 2 if nl > 100 else 0)     # tuples of runs that straddle word and 2048-row edges
    want = check_all_forms(gpu_ctx, tuple_columns(types, lids, rng), tuple_columns(types, rids, rng), f"seams nl {nl} nr {nr}")
    assert 0 < len(want[(I, True)][0].data) and len(want[(I, False)][0].data) < len(want[(U, False)][0].data)


# ---- 2. one tuple in all rows, and n distinct tuples, past one sweep of the bitmap kernels --------------------------------
def test_one_tuple_in_every_row_past_one_sweep(gpu_ctx):
    """min(cL, cR) and cL - cR both end inside a word of the second trip of the stride."""
    cl, cr = 2 * SWEEP + 307, SWEEP + 113
    assert min(cl, cr) > SWEEP and cl - cr > SWEEP and min(cl, cr) % 64 and (cl - cr) % 64
    lcols = [Column(I32, np.full(cl, 7, dtype=np.int32)), Column(D, np.full(cl, NAN))]
    rcols = [Column(I32, np.full(cr, 7, dtype=np.int32)), Column(D, np.full(cr, NAN))]
    want = check_all_forms(gpu_ctx, lcols, rcols, "one tuple")
    assert [len(want[f][0].data) for f in FORMS] == [1, cl + cr, 1, cr, 0, cl - cr]


def test_every_row_its_own_tuple_past_one_sweep(gpu_ctx):
    rng = np.random.default_rng(510)
    n = SWEEP + 77
    ids = rng.permutation(n).astype(np.int32)
    nl = n // 2 + 9
    lcols, rcols = [Column(I32, ids[:nl])], [Column(I32, ids[nl:])]
    want = check_all_forms(gpu_ctx, lcols, rcols, "n distinct tuples")
    assert [len(want[f][0].data) for f in FORMS] == [n, n, 0, 0, nl, nl]


# ---- 3. nullability ------------------------------------------------------------------------------------------------------------
def test_nullability_of_either_side(gpu_ctx):
    """Column 0 is nullable on the left only, 1 on the right only, 2 on both, 3 on neither."""
    rng = np.random.default_rng(520)
    nl, nr = 300, 333

    def side(n, nullable):
        cols = []
        for has in nullable:
            valid = rng.random(n) > 0.4 if has else None
            if valid is not None:
                valid[:2] = [True, False]       # never all ones: the bitmap stays
            cols.append(Column(I32, rng.integers(0, 2, n).astype(np.int32), valid))
        return cols
    lcols, rcols = side(nl, [True, False, True, False]), side(nr, [False, True, True, False])
    want = check_all_forms(gpu_ctx, lcols, rcols, "nullability")
    for cols in want.values():
        assert [w.nullable for w in cols] == [True, True, True, False]
    both = want[(I, False)]
    assert (~both[2].valid).any() and both[0].valid.all() and both[1].valid.all()      # NULL on the right equals NULL on the left


# ---- 4. dictionaries -----------------------------------------------------------------------------------------------------------
LEFT_DICT = ["m", "b", "zz", "a"]
DICTS = {"same-object": (LEFT_DICT, LEFT_DICT), "reordered": (LEFT_DICT, LEFT_DICT[::-1]), "overlapping": (LEFT_DICT, ["a", "q", "zz", "c"]),
         "disjoint": (LEFT_DICT, ["x", "y", "Zü"]), "twice-listed": (["a", "b", "a"], ["b", "x", "b", "y", "a", "x"])}


@pytest.mark.parametrize("mode", list(DICTS))
def test_dictionaries(gpu_ctx, mode):
    rng = np.random.default_rng(530 + list(DICTS).index(mode))
    ld, rd = DICTS[mode]
    nl, nr = 200, 263
    lcols = [Column(S, rng.integers(0, len(ld), nl).astype(np.int32), rng.random(nl) > 0.2, ld), Column(I32, rng.integers(0, 2, nl).astype(np.int32))]
    rcols = [Column(S, rng.integers(0, len(rd), nr).astype(np.int32), rng.random(nr) > 0.2, rd), Column(I32, rng.integers(0, 2, nr).astype(np.int32))]
    lbatch, lres = build(gpu_ctx, lcols)
    rbatch, rres = build(gpu_ctx, rcols)
    try:
        for op, all_ in FORMS:
            want = check_form(gpu_ctx, lcols, rcols, lres, rres, op, all_, mode)
            assert (gpu_ctx.last_set_stats()["translated_columns"] == 0) == (mode == "same-object")
            merged = list(ld) + ([] if mode == "same-object" else [s for s in rd if s not in ld])
            assert want[0].dictionary == merged
        out = gpu_ctx.set_op(lres, rres, U, True)
        got = out.column_to_host(0)
        assert np.array_equal(got.data[:nl], lcols[0].data)                             # left codes come out unchanged
        assert [got.dictionary[c] for c in got.data[nl:]] == [rd[c] for c in rcols[0].data]   # right codes say the same strings
        out.free()
    finally:
        lres.free(); rres.free(); lbatch.free(); rbatch.free()


# ---- 5. identities that do not rest on the reference ---------------------------------------------------------------------------
def test_identities(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(540)
    nl, nr = 2 * T + 19, T + 45
    types = [I32, D, S, B]
    lcols = tuple_columns(types, rng.integers(0, 300, nl), rng)
    rcols = tuple_columns(types, rng.integers(150, 450, nr), rng)
    lbatch, lres = build(ctx, lcols)
    rbatch, rres = build(ctx, rcols)
    everything = list(range(len(types)))
    try:
        # UNION ALL: nL + nR rows, the left's bytes, then the right's
        ua = ctx.set_op(lres, rres, U, True)
        assert ua.count == nl + nr and ctx.last_set_stats() == {"left_rows": nl, "right_rows": nr, "tuples": 0, "translated_columns": 0}
        for g, l, r in zip(ua.to_columns(), lres.to_columns(), rres.to_columns()):
            assert g.data.tobytes() == np.concatenate([l.data, r.data]).tobytes()
            assert np.array_equal(g.valid, np.concatenate([l.valid, r.valid]))
        # |INTERSECT ALL| + |EXCEPT ALL| = nL
        ia, xa = ctx.set_op(lres, rres, I, True), ctx.set_op(lres, rres, X, True)
        assert ia.count + xa.count == nl and ia.count > 0 and xa.count > 0
        # UNION = concat + DISTINCT over every column, byte for byte (one shared dictionary)
        u = ctx.set_op(lres, rres, U)
        tuples = ctx.last_set_stats()["tuples"]
        cat = ctx.concat([lres, rres])
        distinct = ctx.group_ordered(cat, everything, [])
        assert u.count == distinct.count == tuples and column_bytes(u) == column_bytes(distinct)
        # INTERSECT(A, A) = UNION(A, A) = DISTINCT A
        aa_i, aa_u, da = ctx.set_op(lres, lres, I), ctx.set_op(lres, lres, U), ctx.group_ordered(lres, everything, [])
        assert column_bytes(aa_i) == column_bytes(aa_u) == column_bytes(da) and aa_i.count == da.count > 0
        # EXCEPT(A, A): no row, the full schema
        for all_ in (False, True):
            none = ctx.set_op(lres, lres, X, all_)
            assert none.count == 0 and none.ncols == len(types)
            assert [DataType(none.view(c).type) for c in everything] == types and all(none.view(c).nullable for c in everything)
            assert none.column_to_host(2).dictionary == STRINGS
            none.free()
        for r in (ua, ia, xa, u, cat, distinct, aa_i, aa_u, da):
            r.free()
    finally:
        lres.free(); rres.free(); lbatch.free(); rbatch.free()


# ---- 6. eight columns (the sort's limit) and one column --------------------------------------------------------------------------
def test_eight_columns_and_one_column(gpu_ctx):
    rng = np.random.default_rng(550)
    nl, nr = 700, 650
    types = [B, S, I32, D, I64, B, S, D]
    lids, rids = rng.integers(0, 90, nl), rng.integers(30, 120, nr)
    want = check_all_forms(gpu_ctx, tuple_columns(types, lids, rng), tuple_columns(types, rids, rng), "eight columns")
    assert len(want[(I, False)]) == 8 and 0 < len(want[(I, False)][0].data) < len(want[(U, False)][0].data)
    for t in (D, B, S):
        one_l, one_r = tuple_columns([t], lids, rng)[:1], tuple_columns([t], rids, rng)[:1]
        check_all_forms(gpu_ctx, one_l, one_r, f"one {t.name} column")


# ---- 7. empty sides ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", ["left", "right", "both"])
def test_empty_sides(gpu_ctx, empty):
    rng = np.random.default_rng(560)
    types = [S, D, B, I64]
    full = tuple_columns(types, rng.integers(0, 40, 130), rng)
    none = [Column(c.type, c.data[:0], None, c.dictionary) for c in full]
    lcols, rcols = (none if empty in ("left", "both") else full), (none if empty in ("right", "both") else full)
    want = check_all_forms(gpu_ctx, lcols, rcols, f"{empty} empty")
    counts = [len(want[f][0].data) for f in FORMS]
    distinct = len(want[(U, False)][0].data)
    assert (distinct == 0) if empty == "both" else (1 < distinct < 130)
    assert counts == {"left": [distinct, 130, 0, 0, 0, 0], "right": [distinct, 130, 0, 0, distinct, 130], "both": [0] * 6}[empty]
    assert all(len(cols) == 4 for cols in want.values())


# ---- 8. the operator among the others -------------------------------------------------------------------------------------------
def test_chaining_with_the_inputs_freed_first(gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(570)
    nl, nr = 3000, 2500
    lcols = [Column(I32, rng.integers(0, 40, nl).astype(np.int32)), Column(D, rng.integers(0, 6, nl) / 2.0, rng.random(nl) > 0.1)]
    rcols = [Column(I32, rng.integers(10, 50, nr).astype(np.int32)), Column(D, rng.integers(0, 6, nr) / 2.0, rng.random(nr) > 0.1)]
    want, _ = setop_reference(lcols, rcols, [False, True], [False, True], I, True)
    lbatch, lres = build(ctx, lcols)
    rbatch, rres = build(ctx, rcols)
    out = ctx.set_op(lres, rres, I, True)
    lres.free(); rres.free(); lbatch.free(); rbatch.free()          # the output owns its buffers
    assert_window_output(out, want, "after the inputs were freed")
    # into a GROUP BY through as_batch()
    obatch = out.as_batch()
    key = ColumnExpression("k", 0, I32)
    grouped = E.filter_groupby(ctx, obatch, None, [ctx.compile(key)], [ctx.compile(key)], [int(AF.COUNT)])
    g = grouped.to_columns()
    keys, counts = np.unique(want[0].data, return_counts=True)
    order = np.argsort(g[0].data)
    assert grouped.count == len(keys) and np.array_equal(g[0].data[order], keys) and np.array_equal(g[1].data[order], counts.astype(np.float64))
    # through ORDER BY (descending on the key: the reversed rows, ties in their order)
    by_key = ctx.order_by_keys(out, [(0, True)])
    assert by_key.count == out.count and np.all(np.diff(by_key.column_to_host(0).data) <= 0)
    # into a second set operation, with itself and with another result
    again = ctx.set_op(out, by_key, X, True)
    assert again.count == 0 and again.ncols == 2
    distinct = ctx.set_op(out, out, U)
    want_distinct, _ = setop_reference([Column(w.type, w.data, w.valid) for w in want], [Column(w.type, w.data, w.valid) for w in want],
                                       [False, True], [False, True], U, False)
    assert_window_output(distinct, want_distinct, "a second set operation")
    for r in (distinct, again, by_key, grouped, obatch, out):
        r.free()


def test_operator_on_gpu_sources_matches_its_host_branch(gpu_ctx):
    from queryengine_amd import ColumnarTable, Field, Schema
    from queryengine_amd.operators import GpuFilterProjectOperator, SetOperator, map as op_map
    from test_setop_cpu import Rows, assert_rows
    rng = np.random.default_rng(571)

    def table(n, dictionary):
        cols = [Column(S, rng.integers(0, len(dictionary), n).astype(np.int32), rng.random(n) > 0.2, dictionary),
                Column(D, np.array([NAN, -0.0, 0.0, 1.5])[rng.integers(0, 4, n)], rng.random(n) > 0.2)]
        return cols, ColumnarTable(Schema([Field("k", S), Field("v", D)]), cols)
    (lcols, ltable), (rcols, rtable) = table(150, ["a", "b", "c"]), table(170, ["c", "d", "a"])
    exprs = [ColumnExpression("k", 0, S), ColumnExpression("v", 1, D)]
    for op, all_ in FORMS:
        left = GpuFilterProjectOperator(gpu_ctx, ltable.getScanOperator(["k", "v"]), None, exprs)
        right = GpuFilterProjectOperator(gpu_ctx, rtable.getScanOperator(["k", "v"]), None, exprs)
        dev = op_map(SetOperator(left, right, op, all_), list)
        host = op_map(SetOperator(Rows([[c.value(i) for c in lcols] for i in range(150)]), Rows([[c.value(i) for c in rcols] for i in range(170)]),
                                  op, all_), list)
        assert_rows(dev, host, f"{NAMES[op]} all {all_}")


@pytest.mark.parametrize("nl, nr", [(1, 0), (0, 1), (1, 1), (40, 24), (40, 25), (600, 425)], ids=lambda v: str(v))
def test_small_totals_against_the_host_operator(gpu_ctx, nl, nr):
    """nl + nr = 1, 2, 64, 65 (the word edge of the tuple-start bitmap) and 1025 (past one 1024-row block of the radix
    histogram), over a nullable STRING column whose sides carry different dictionaries that share some strings."""
    from queryengine_amd.operators import SetOperator, map as op_map
    from test_setop_cpu import Rows, assert_rows
    rng = np.random.default_rng(575 + nl + nr)

    def side(n, dictionary):
        valid = rng.random(n) > 0.2 if n else None
        if n > 1:
            valid[:2] = [True, False]       # never all ones: the bitmap stays
        return [Column(S, rng.integers(0, len(dictionary), n).astype(np.int32), valid, dictionary), Column(I32, rng.integers(0, 3, n).astype(np.int32))]
    lcols, rcols = side(nl, ["m", "b", "zz", "a"]), side(nr, ["a", "q", "zz", "c"])
    boxed = lambda cols, n: [[c.value(i) for c in cols] for i in range(n)]      # noqa: E731
    lbatch, lres = build(gpu_ctx, lcols)
    rbatch, rres = build(gpu_ctx, rcols)
    try:
        tuples = len(op_map(SetOperator(Rows(boxed(lcols, nl)), Rows(boxed(rcols, nr)), U), list))
        for op, all_ in FORMS:
            host = op_map(SetOperator(Rows(boxed(lcols, nl)), Rows(boxed(rcols, nr)), op, all_), list)
            out = gpu_ctx.set_op(lres, rres, op, all_)
            try:
                assert_rows(boxed(out.to_columns(), out.count), host, f"nl {nl} nr {nr} {NAMES[op]} all {all_}")
                assert gpu_ctx.last_set_stats() == {"left_rows": nl, "right_rows": nr, "tuples": 0 if (op == U and all_) else tuples,
                                                    "translated_columns": 1}
            finally:
                out.free()
    finally:
        lres.free(); rres.free(); lbatch.free(); rbatch.free()


# ---- 9. determinism ------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_on_every_run_and_on_a_fresh_context(gpu_ctx):
    rng = np.random.default_rng(580)
    nl, nr = 3 * T + 5, 2 * T + 71
    types = [D, S, B, I32]
    lcols, rcols = tuple_columns(types, rng.integers(0, 500, nl), rng), tuple_columns(types, rng.integers(200, 700, nr), rng, dictionary=STRINGS[::-1])

    def run(ctx):
        lbatch, lres = build(ctx, lcols)
        rbatch, rres = build(ctx, rcols)
        data = []
        for op, all_ in FORMS:
            out = ctx.set_op(lres, rres, op, all_)
            data.append(column_bytes(out))
            out.free()
        lres.free(); rres.free(); lbatch.free(); rbatch.free()
        return data

    first = run(gpu_ctx)
    assert run(gpu_ctx) == first
    other = E.Context(device=0)
    try:
        assert run(other) == first
    finally:
        other.close()


# ---- 10. errors ----------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_and_limits(gpu_ctx):
    ctx = gpu_ctx
    lib = ctx._lib
    rng = np.random.default_rng(590)
    n = 50
    cols = [Column(I32, rng.integers(0, 5, n).astype(np.int32)), Column(D, rng.normal(0, 1, n)), Column(S, rng.integers(0, 3, n).astype(np.int32), None, STRINGS)]
    batch, res = build(ctx, cols)
    fewer_batch, fewer = build(ctx, cols[:2])
    other_batch, other = build(ctx, [cols[0], Column(I64, np.arange(n, dtype=np.int64)), cols[2]])
    nine = [Column(I32, rng.integers(0, 3, n).astype(np.int32)) for _ in range(9)]
    nine_batch, nine_res = build(ctx, nine)
    table = ctx.join_build(nine_res, [0])                     # a SEMI join lists probe columns twice: a result of 17 columns
    seventeen = table.probe(nine_res, [0], N.JOIN_SEMI, list(range(9)) + list(range(8)), [])
    assert seventeen.ncols == 17 and seventeen.count == n

    def call(left=res, right=res, op=U, all_=0, null=()):
        out = C.c_void_p(0xdead)
        st = lib.qe_result_set_op(None if "ctx" in null else ctx.handle, None if "left" in null else left.handle,
                                  None if "right" in null else right.handle, op, all_, None if "out" in null else C.byref(out))
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
        assert call(op=3) == INVALID_ARG and call(op=-1) == INVALID_ARG
        assert call(all_=2) == INVALID_ARG and call(all_=-1) == INVALID_ARG
        assert call(right=fewer) == INVALID_ARG and call(left=fewer) == INVALID_ARG           # different column counts
        assert call(right=other) == INVALID_ARG                                               # a column whose types differ
        for op, all_ in FORMS:                                                                # nine columns: past the sort's keys
            assert call(left=nine_res, right=nine_res, op=op, all_=int(all_)) == (N.OK if (op, all_) == (U, True) else UNSUPPORTED)
        assert call(left=seventeen, right=seventeen, op=U, all_=1) == UNSUPPORTED             # the limit of qe_result_concat
        check_form(ctx, cols, cols, res, res, X, True, "after the errors")                    # the context still works
        ua = ctx.set_op(nine_res, nine_res, U, True)
        assert ua.count == 2 * n and ua.ncols == 9
        ua.free()
    finally:
        table.free()
        for r in (res, fewer, other, nine_res, seventeen, batch, fewer_batch, other_batch, nine_batch):
            r.free()
