"""qe_result_order_by_keys on the device: several keys, ASC / DESC, LIMIT as a top-k selection.

The expectation is always the host branch of ``OrderByOperator`` (one stable ``list.sort`` per key from the last to the
first with ``_compare_key``, ``reverse=True`` for a descending key, then the slice): Kotlin's
``compareBy().thenByDescending()`` on a stable ``sortWith``.  The reference has one ascending key and no LIMIT, so this
parity is not pinned by reference fixtures.  Every result carries an INT64 row id, and the row-id column is compared
exactly: it fixes the order including the ties."""
import ctypes as C
import itertools

import numpy as np
import pytest

from queryengine_amd import Column, ColumnarTable, ColumnExpression, DataType, Field, Schema, TableRegistry
from queryengine_amd import engine as E
from queryengine_amd import native as N
from queryengine_amd.operators import Operator, OrderByOperator, map as op_map
from queryengine_amd.planner import Mode, query

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
STRINGS = ["b", "a", "", "B", "～", "\U0001F600", "aa", "Zü", "zz", "a "]
DOUBLES = np.array([0.0, -0.0, 1.5, -1.5, float("nan"), float("inf"), -float("inf"), 1e300, -1e-300, 3.0])
INVALID_ARG = 1          # QE_ERR_INVALID_ARG
INT64S = np.array([0, -1, 1, 2 ** 63 - 1, -(2 ** 63), 2 ** 53 + 1, 2 ** 63 - 2], dtype=np.int64)


class Rows(Operator):
    """A plain row source: OrderByOperator sorts it on the host."""

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


def make_key(t, rng, n, coarse, null_share=0.05):
    """A key column of type t with the special-value pools; coarse = tens of distinct values."""
    valid = rng.random(n) >= null_share if null_share > 0 else None
    if t == D:
        data = DOUBLES[rng.integers(0, len(DOUBLES), n)]
        if not coarse:
            data = np.where(rng.random(n) < 0.5, data, rng.normal(0, 1e3, n))
        return Column(D, data, valid)
    if t == I64:
        data = INT64S[rng.integers(0, len(INT64S), n)]
        return Column(I64, data if coarse else np.where(rng.random(n) < 0.3, data, rng.integers(-5000, 5000, n)), valid)
    if t == I32:
        return Column(I32, (rng.integers(-8, 8, n) if coarse else rng.integers(-2 ** 31, 2 ** 31 - 1, n)).astype(np.int32), valid)
    if t == S:
        return Column(S, rng.integers(0, len(STRINGS), n).astype(np.int32), valid, STRINGS)
    return Column(B, rng.random(n) > 0.5, valid)


def build(ctx, keycols, rng):
    """filter_project over an identity projection: (key columns.., INT64 row id, nullable BOOLEAN payload)."""
    n = len(keycols[0])
    rowid = Column(I64, np.arange(n, dtype=np.int64))
    flag = Column(B, rng.random(n) > 0.3, (rng.random(n) > 0.2) if n else None)
    cols = list(keycols) + [rowid, flag]
    batch = E.DeviceBatch.from_columns(ctx, cols)
    projs = [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)]
    return batch, E.filter_project(ctx, batch, None, projs), cols


def host_order(cols, keys, limit=None):
    """Row ids in the order of the host branch of OrderByOperator."""
    n = len(cols[0])
    ncol = max(c for c, _ in keys) + 1
    values = [[cols[c].value(i) for i in range(n)] if any(c == kc for kc, _ in keys) else None for c in range(ncol)]
    rows = [[values[c][i] if values[c] is not None else None for c in range(ncol)] + [i] for i in range(n)]
    return op_map(OrderByOperator(Rows(rows), keys[0][0], keys, limit), lambda r: r[-1])


def same_value(a, b):
    return a == b or (a != a and b != b)


def check(ctx, res, cols, keys, limit=None, want=None):
    n = len(cols[0])
    if want is None:
        want = host_order(cols, keys, limit)
    srt = ctx.order_by_keys(res, keys, limit)
    try:
        out = srt.to_columns()
        assert srt.count == len(want) == (n if limit is None else min(limit, n))
        rid = len(cols) - 2
        assert np.array_equal(out[rid].data, np.array(want, dtype=np.int64)), (keys, limit, ctx.last_sort_stats())
        m = len(want)
        for j in sorted({0, 1, m // 3, m // 2, m - 2, m - 1} & set(range(m))):
            for c in range(len(cols)):
                assert same_value(out[c].value(j), cols[c].value(want[j])), (keys, limit, j, c)
    finally:
        srt.free()
    return want


PAIRS = [(D, S), (I64, B), (S, D), (B, I32), (I32, I64)]


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0].name}-{p[1].name}")
def test_two_keys_in_every_direction(gpu_ctx, pair):
    rng = np.random.default_rng(11)
    n = 200_003
    cols = [make_key(pair[0], rng, n, coarse=True), make_key(pair[1], rng, n, coarse=False)]
    batch, res, cols = build(gpu_ctx, cols, rng)
    for d0, d1 in itertools.product((False, True), repeat=2):
        check(gpu_ctx, res, cols, [(0, d0), (1, d1)])
    res.free(); batch.free()


def test_three_keys_with_a_repeated_column_and_an_all_null_key(gpu_ctx):
    rng = np.random.default_rng(12)
    n = 50_021
    nulls = Column(D, np.zeros(n), np.zeros(n, dtype=bool))
    cols = [make_key(I32, rng, n, coarse=True), make_key(S, rng, n, coarse=True), nulls]
    batch, res, cols = build(gpu_ctx, cols, rng)
    check(gpu_ctx, res, cols, [(0, True), (1, False), (0, False)])
    check(gpu_ctx, res, cols, [(1, True), (0, True), (1, True)])
    want = check(gpu_ctx, res, cols, [(2, False)])
    assert want == list(range(n))                         # all NULL: nothing moves
    check(gpu_ctx, res, cols, [(2, True), (0, False)])
    check(gpu_ctx, res, cols, [(2, True)], limit=10)
    res.free(); batch.free()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_word_and_block_boundaries(gpu_ctx, n):
    rng = np.random.default_rng(100 + n)
    cols = [make_key(D, rng, n, coarse=True), make_key(I64, rng, n, coarse=False)]
    batch, res, cols = build(gpu_ctx, cols, rng)
    for d0, d1 in itertools.product((False, True), repeat=2):
        check(gpu_ctx, res, cols, [(0, d0), (1, d1)])
        check(gpu_ctx, res, cols, [(0, d0), (1, d1)], limit=3)
    res.free(); batch.free()


@pytest.mark.parametrize("t", [D, I64, I32, S, B], ids=lambda t: t.name)
def test_one_ascending_key_returns_the_bytes_of_order_by(gpu_ctx, t):
    rng = np.random.default_rng(13)
    n = 100_003
    batch, res, cols = build(gpu_ctx, [make_key(t, rng, n, coarse=False)], rng)
    a = gpu_ctx.order_by(res, 0)
    b = gpu_ctx.order_by_keys(res, [(0, False)])
    assert a.count == b.count == n
    for ca, cb in zip(a.to_columns(), b.to_columns()):
        assert ca.type == cb.type
        assert ca.data.tobytes() == cb.data.tobytes()
        assert (ca.valid is None) == (cb.valid is None)
        if ca.valid is not None:
            assert ca.valid.tobytes() == cb.valid.tobytes()
    a.free(); b.free(); res.free(); batch.free()


def test_top_k_of_distinct_doubles_selects_on_the_device(gpu_ctx):
    rng = np.random.default_rng(14)
    n = 2_000_003
    key = Column(D, rng.permutation(n).astype(np.float64) / n + rng.integers(0, 3, n) * 7.0)     # distinct values
    assert len(np.unique(key.data)) == n
    batch, res, cols = build(gpu_ctx, [key], rng)
    for desc in (False, True):
        full = host_order(cols, [(0, desc)])
        for k in (0, 1, 7, 64, 1000, n - 1, n, n + 5):
            check(gpu_ctx, res, cols, [(0, desc)], limit=k, want=full[:k])
            st = gpu_ctx.last_sort_stats()
            if 0 < k <= 1000:
                assert st["path"] == "select", st
                assert st["sorted_rows"] <= n // 16, st
                assert st["select_passes"] <= 8, st
    res.free(); batch.free()


def stable_order(key, desc, limit=None):
    """Row ids of a nullable INT32 key in the documented order, as a numpy stable argsort: ascending NULL first,
    descending NULL last, ties in row order."""
    v = key.data.astype(np.int64)
    valid = key.valid if key.valid is not None else np.ones(len(v), dtype=bool)
    image = np.where(valid, -v if desc else v, 2 ** 40 if desc else -2 ** 40)
    order = np.argsort(image, kind="stable")
    return order if limit is None else order[:limit]


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
def test_sort_past_the_grid_cap_is_stable(gpu_ctx, desc):
    """8192 x 256 + 65 rows: sort_key_kernel, gather_rows_kernel (4 and 8 bytes) and gather_bits_rows_kernel run their
    stride loops; tens of distinct key values, so stability decides almost every position.  The row-id column and the
    nullable BOOLEAN column are compared in full."""
    rng = np.random.default_rng(21)
    n = 8192 * 256 + 65
    key = Column(I32, rng.integers(-20, 20, n).astype(np.int32), rng.random(n) >= 0.05)
    head = Column(I32, key.data[:5000], key.valid[:5000])                        # the numpy order IS the host branch's order
    for limit in (None, 100):
        assert stable_order(head, desc, limit).tolist() == host_order([head], [(0, desc)], limit)
    batch, res, cols = build(gpu_ctx, [key], rng)
    flag = cols[2]
    assert flag.valid is not None and len(np.unique(key.data)) == 40
    for limit in (None, 100):
        want = stable_order(key, desc, limit)
        assert want.max() >= 8192 * 256 or limit is not None                     # rows of the second stride take part
        srt = gpu_ctx.order_by_keys(res, [(0, desc)], limit)
        try:
            out = srt.to_columns()
            assert srt.count == len(want) == (n if limit is None else limit)
            assert np.array_equal(out[1].data, want), (desc, limit, gpu_ctx.last_sort_stats())
            for c in (0, 2):                                                     # the key and the flag, every row
                gv = out[c].valid if out[c].valid is not None else np.ones(len(want), dtype=bool)
                assert np.array_equal(gv, cols[c].valid[want]), (desc, limit, c)
                assert np.array_equal(out[c].data[gv], cols[c].data[want][gv]), (desc, limit, c)
        finally:
            srt.free()
    res.free(); batch.free()


def test_top_k_across_a_tie(gpu_ctx):
    rng = np.random.default_rng(15)
    n = 300_007
    first = Column(I32, rng.integers(0, 10, n).astype(np.int32))                 # 10 distinct values
    cols = [first, make_key(D, rng, n, coarse=False)]
    batch, res, cols = build(gpu_ctx, cols, rng)
    k = int(np.sum(first.data < 3) + np.sum(first.data == 3) // 2)               # in the middle of the run of 3
    for desc in (False, True):
        kk = k if not desc else int(np.sum(first.data > 6) + np.sum(first.data == 6) // 2)
        check(gpu_ctx, res, cols, [(0, desc)], limit=kk)
        check(gpu_ctx, res, cols, [(0, desc), (1, True)], limit=kk)
    check(gpu_ctx, res, cols, [(0, False)], limit=17)                            # inside the first run: c = a tenth of n
    res.free(); batch.free()


def test_top_k_on_a_boolean_first_key(gpu_ctx):
    rng = np.random.default_rng(16)
    n = 100_019
    cols = [make_key(B, rng, n, coarse=True), make_key(I64, rng, n, coarse=False)]
    batch, res, cols = build(gpu_ctx, cols, rng)
    for desc in (False, True):
        for k in (5, 1000, n // 3):
            check(gpu_ctx, res, cols, [(0, desc), (1, False)], limit=k)
            check(gpu_ctx, res, cols, [(0, desc)], limit=k)
    res.free(); batch.free()


def test_top_k_and_the_null_class(gpu_ctx):
    """ASC: the k smallest are all NULL; DESC: the NULLs fall beyond k."""
    rng = np.random.default_rng(17)
    n = 200_003
    key = Column(D, rng.random(n), rng.random(n) >= 0.02)                        # ~4000 NULLs
    nnull = int(np.sum(~key.valid))
    batch, res, cols = build(gpu_ctx, [key, make_key(I32, rng, n, coarse=True)], rng)
    for k in (1, 100, nnull - 1, nnull, nnull + 1, nnull + 50):
        check(gpu_ctx, res, cols, [(0, False)], limit=k)
        check(gpu_ctx, res, cols, [(0, False), (1, True)], limit=k)
    for k in (1, 100, 5000, n - nnull - 1, n - nnull, n - nnull + 1):
        check(gpu_ctx, res, cols, [(0, True)], limit=k)
    # INT64 extremes share their image with the NULL class of the selection: they must still come after / before it
    ext = Column(I64, np.where(rng.random(n) < 0.01, np.int64(-(2 ** 63)), rng.integers(-9, 9, n)), rng.random(n) >= 0.01)
    ext.data[rng.random(n) < 0.01] = 2 ** 63 - 1
    batch2, res2, cols2 = build(gpu_ctx, [ext], rng)
    nn = int(np.sum(~ext.valid))
    for k in (nn - 3, nn, nn + 3, nn + 500):
        check(gpu_ctx, res2, cols2, [(0, False)], limit=k)
        check(gpu_ctx, res2, cols2, [(0, True)], limit=k)
    res2.free(); batch2.free(); res.free(); batch.free()


def test_top_k_on_skewed_first_keys(gpu_ctx):
    """Guards the per-wave histogram: a sorted key and a key that is one value in 99 % of the rows put whole waves on one bin."""
    rng = np.random.default_rng(18)
    n = 400_009
    srt = Column(I64, np.arange(n, dtype=np.int64) // 3 - 1000)
    skew = Column(D, np.where(rng.random(n) < 0.99, 42.0, rng.normal(0, 100, n)))
    batch, res, cols = build(gpu_ctx, [srt, skew], rng)
    for c in (0, 1):
        for desc in (False, True):
            check(gpu_ctx, res, cols, [(c, desc)], limit=100)
    check(gpu_ctx, res, cols, [(1, False), (0, True)], limit=100)
    res.free(); batch.free()


@pytest.mark.parametrize("mode", [Mode.GPU_FUSED, Mode.GPU_PER_NODE])
def test_order_by_desc_limit_through_sql(mode, gpu_ctx, gpu_ctx_per_node):
    ctx = gpu_ctx if mode == Mode.GPU_FUSED else gpu_ctx_per_node
    rng = np.random.default_rng(19)
    n = 30_000
    a = rng.integers(0, 1000, n).astype(np.float64)
    c = np.round(rng.random(n), 2)                                               # ties on the first key
    names = ["DE", "AT", "CH", "FR", "IT", "ES"]
    s = Column(S, rng.integers(0, len(names), n).astype(np.int32) % rng.integers(1, 7, n).astype(np.int32), None, names)
    t = ColumnarTable(Schema([Field("a", D), Field("c", D), Field("s", S)]), [Column(D, a), Column(D, c, rng.random(n) > 0.1), s])
    reg = TableRegistry()
    reg.register("t", t)
    rows = query(reg, "SELECT a + 1, c FROM t WHERE a < 500 ORDER BY 2 DESC, 1 LIMIT 25", mode, ctx=ctx)
    cv = t.columns[1]
    exp = [[a[i] + 1, cv.value(i)] for i in np.nonzero(a < 500)[0]]
    exp = op_map(OrderByOperator(Rows(exp), 1, [(1, True), (0, False)], 25), lambda r: r)
    assert rows == exp and len(rows) == 25 and rows[0][1] is not None
    assert ctx.last_sort_stats()["path"] == "select"
    rows = query(reg, "SELECT s, SUM(a) FROM t ORDER BY 2 DESC LIMIT 3", mode, ctx=ctx)
    sums = {}
    for i in range(n):
        sums[s.value(i)] = sums.get(s.value(i), 0.0) + a[i]
    top = sorted(sums.items(), key=lambda kv: -kv[1])[:3]
    assert [r[0] for r in rows] == [k for k, _ in top]
    assert [r[1] for r in rows] == pytest.approx([v for _, v in top], rel=1e-12)


def test_invalid_arguments_leave_the_context_usable(gpu_ctx, native_lib):
    rng = np.random.default_rng(20)
    batch, res, cols = build(gpu_ctx, [make_key(I32, rng, 1000, coarse=True)], rng)
    lib = native_lib

    def call(keys, nkeys, null_keys=False):
        arr = (N.SortKey * 9)(*[N.SortKey(c, d) for c, d in keys])
        out = C.c_void_p(0xdead)
        st = lib.qe_result_order_by_keys(gpu_ctx.handle, res.handle, None if null_keys else arr, nkeys, -1, C.byref(out))
        assert out.value is None
        return st

    assert call([(0, 0)], 0) == INVALID_ARG
    assert call([(0, 0)] * 9, 9) == INVALID_ARG
    assert call([(3, 0)], 1) == INVALID_ARG
    assert call([(0, 0), (-1, 1)], 2) == INVALID_ARG
    assert call([(0, 0)], 1, null_keys=True) == INVALID_ARG
    assert lib.qe_result_order_by_keys(gpu_ctx.handle, None, (N.SortKey * 1)(), 1, -1, C.byref(C.c_void_p())) == INVALID_ARG
    assert lib.qe_result_order_by_keys(gpu_ctx.handle, res.handle, (N.SortKey * 1)(), 1, -1, None) == INVALID_ARG
    check(gpu_ctx, res, cols, [(0, True)], limit=10)                             # the context still works
    check(gpu_ctx, res, cols, [(0, False)] * 8)                                  # 8 keys are allowed
    res.free(); batch.free()
