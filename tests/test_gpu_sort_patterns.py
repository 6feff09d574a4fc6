"""The shared radix sort and the top-k select under PLACED key images.

Random key pools vary in every nibble or only in the lowest one, never put a whole radix block on one digit, and reach the
equalities of the select's rank walk and stop rule only by accident.  Here the images are placed (sort_pattern_reference.py,
whose properties test_sort_patterns_cpu.py pins down) and every call is compared three ways: the row-id column with the
numpy order in full, every other column in full (values and validity), and last_sort_stats() with the host model -- path,
rows sorted, radix passes, selection passes."""
import contextlib
import itertools

import numpy as np
import pytest

from queryengine_amd import Column, ColumnExpression, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N

import sort_pattern_reference as R

pytestmark = pytest.mark.gpu
D, I64, I32, B = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN
N_SKIP = 3 * 1024 + 1
DIRECTIONS = (False, True)


@contextlib.contextmanager
def built(ctx, keycols, seed=0):
    """filter_project over an identity projection: (key columns.., INT64 row id, nullable BOOLEAN payload).  Yields (result,
    host columns); the result and its batch are freed on the way out, also past a failing assertion."""
    rng = np.random.default_rng(seed)
    n = len(keycols[0])
    rowid = Column(I64, np.arange(n, dtype=np.int64))
    flag = Column(B, rng.random(n) > 0.3, rng.random(n) > 0.2)
    cols = list(keycols) + [rowid, flag]
    batch = E.DeviceBatch.from_columns(ctx, cols)
    res = None
    try:
        projs = [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)]
        res = E.filter_project(ctx, batch, None, projs)
        for i, c in enumerate(cols):      # the pass count of the reference rests on this: a bitmap given is a bitmap kept
            assert (res.view(i).validity is not None) == (c.valid is not None), i
        yield res, cols
    finally:
        if res is not None:
            res.free()
        batch.free()


def raw(column, rows):
    """Bytes-exact values of `column` at `rows` (a DOUBLE by its bits: NaN payloads must come through) and their validity."""
    data = column.data.view(np.uint64) if column.type == D else column.data
    valid = np.ones(len(column), dtype=bool) if column.valid is None else column.valid
    return data[rows], valid[rows]


def check(ctx, res, cols, keys, limit=None):
    """One order_by_keys call: rows, columns, stats."""
    n = len(cols[0])
    want = R.expected_order(cols, keys, limit)
    stats = R.expected_stats(cols, keys, limit)
    srt = ctx.order_by_keys(res, keys, limit)
    try:
        got_stats = ctx.last_sort_stats()
        out = srt.to_columns()
        assert srt.count == len(want) == (n if limit is None else min(limit, n))
        rid = len(cols) - 2
        assert np.array_equal(out[rid].data, want), (keys, limit, got_stats, stats)
        everything = np.arange(len(want))
        for c in range(len(cols)):
            data, valid = raw(cols[c], want)
            got, got_valid = raw(out[c], everything)
            assert np.array_equal(got_valid, valid), (keys, limit, c)
            assert np.array_equal(got[valid], data[valid]), (keys, limit, c)
        assert got_stats == stats, (keys, limit)
    finally:
        srt.free()
    return stats


def nulls_over(images, rng, share=0.1):
    """A nullable INT64 key over the images with garbage under its NULLs (a NULL's image is 0 whatever the data says)."""
    valid = rng.random(len(images)) >= share
    valid[:2] = (False, True)
    return R.int64_key(np.where(valid, images, R.ONES), valid)


def skip_case(ctx, images, nibbles):
    """ASC and DESC on a non-nullable key (constant bits from BASE) and on a nullable one (constant bits 0, like its NULLs)."""
    rng = np.random.default_rng(39)
    plain = R.int64_key(images | np.uint64(R.BASE & ~sum(15 << 4 * d for d in nibbles)))
    with built(ctx, [plain, nulls_over(images, rng)]) as (res, cols):
        for desc in DIRECTIONS:
            assert check(ctx, res, cols, [(0, desc)])["radix_passes"] == len(nibbles)
            assert check(ctx, res, cols, [(1, desc)])["radix_passes"] == len(nibbles) + 1


# ---- skipped passes --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", range(16))
def test_one_varying_nibble(gpu_ctx, d):
    skip_case(gpu_ctx, R.one_nibble(N_SKIP, d, np.random.default_rng(40 + d)), [d])


@pytest.mark.parametrize("b", [0, 3, 4, 31, 32, 59, 60, 63])
def test_one_varying_bit(gpu_ctx, b):
    skip_case(gpu_ctx, R.one_bit(N_SKIP, b, np.random.default_rng(60 + b)), [b // 4])


@pytest.mark.parametrize("a, b", [(0, 15), (7, 8)])
def test_two_varying_nibbles(gpu_ctx, a, b):
    skip_case(gpu_ctx, R.two_nibbles(N_SKIP, a, b, np.random.default_rng(70 + a)), [a, b])


def test_int32_key_that_varies_in_bit_31_only(gpu_ctx):
    rng = np.random.default_rng(80)
    key = Column(I32, np.where(rng.random(N_SKIP) < 0.5, -(2 ** 31) + 5, 5).astype(np.int32))
    with built(gpu_ctx, [key, R.with_validity(Column(I32, key.data.copy()), rng.random(N_SKIP) > 0.1)]) as (res, cols):
        for c, desc in itertools.product((0, 1), DIRECTIONS):
            check(gpu_ctx, res, cols, [(c, desc)])            # the pass count is the reference image's: sign extension and all


# ---- block, round and wave seams -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2048, 2049, 65535, 65536, 65537])
def test_digit_layouts_at_block_and_scan_seams(gpu_ctx, n):
    """Sixteen key values only, so stability decides every position; 65 536 rows fill one trip of the histogram scan."""
    names = list(R.LAYOUTS)
    with built(gpu_ctx, [R.int64_key(R.layout(name, n, d=(3 * j) % 16, base=R.BASE)) for j, name in enumerate(names)], seed=n) as (res, cols):
        for j, name in enumerate(names):
            for desc in DIRECTIONS:
                stats = check(gpu_ctx, res, cols, [(j, desc)])
                assert stats["radix_passes"] == (0 if name == "block_constant" and n <= 1024 else 1), (name, stats)


# ---- NULL placement ---------------------------------------------------------------------------------------------------------

N_NULL = 4 * 1024 + 1


def null_patterns(n):
    i = np.arange(n)
    edges = np.ones(n, dtype=bool)
    edges[(i % 1024 == 0) | (i % 1024 == 1023) | np.isin(i, (63, 64, 255, 256))] = False
    return {"none": np.ones(n, dtype=bool), "all": np.zeros(n, dtype=bool), "blocks": (i // 1024) % 2 == 0, "edges": edges}


@pytest.mark.parametrize("pattern", ["none", "all", "blocks", "edges"])
def test_null_placement(gpu_ctx, pattern):
    valid = null_patterns(N_NULL)[pattern]
    digits = R.layout("lane_cyclic", N_NULL, d=5)
    with built(gpu_ctx, [R.int64_key(digits, valid), R.int64_key(R.layout("wave_cyclic", N_NULL, d=2))], seed=5) as (res, cols):
        assert cols[0].valid is not None                      # also with no NULL: the validity pass runs over all ones
        for desc in DIRECTIONS:
            stats = check(gpu_ctx, res, cols, [(0, desc)])
            assert stats["radix_passes"] == (1 if pattern == "all" else 2), stats
            check(gpu_ctx, res, cols, [(1, not desc), (0, desc)])


def test_int64_extremes_share_their_image_with_null(gpu_ctx):
    """ASC: INT64 min has image 0 like NULL and must follow it; DESC: its image is all ones like NULL's and it must come first."""
    rng = np.random.default_rng(81)
    n = N_NULL
    data = rng.choice(np.array([-(2 ** 63), 2 ** 63 - 1, -(2 ** 63) + 1, 2 ** 63 - 2], dtype=np.int64), n)
    key = R.with_validity(Column(I64, data), rng.random(n) > 0.3)
    with built(gpu_ctx, [key], seed=6) as (res, cols):
        for desc in DIRECTIONS:
            want = R.expected_order(cols, [(0, desc)])
            nnull = int(np.sum(~key.valid))
            null_rows = want[:nnull] if not desc else want[n - nnull:]
            assert not key.valid[null_rows].any() and (np.diff(null_rows) > 0).all()
            check(gpu_ctx, res, cols, [(0, desc)])
            for k in (nnull - 1, nnull, nnull + 1):
                check(gpu_ctx, res, cols, [(0, desc)], limit=k)


# ---- NaN patterns -------------------------------------------------------------------------------------------------------------

NAN_BITS = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF8000000000000, 0xFFF800000000BEEF,
                     0x7FF0000000000001, 0xFFF0000000000001, 0x7FF4000000000000], dtype=np.uint64)      # quiet, payload, sign, signalling
OTHER_BITS = np.array([0.0, -0.0, 5e-324, -5e-324, np.inf, -np.inf, 1.5, -2.5]).view(np.uint64)


def nan_key(n=2049):
    rng = np.random.default_rng(82)
    bits = np.where(rng.random(n) < 0.5, NAN_BITS[rng.integers(0, len(NAN_BITS), n)], OTHER_BITS[rng.integers(0, len(OTHER_BITS), n)])
    return R.double_key(bits, rng.random(n) > 0.1)


def test_every_nan_pattern_is_one_greatest_value(gpu_ctx):
    key = nan_key()
    n = len(key)
    nan = np.isnan(key.data) & key.valid
    with built(gpu_ctx, [key], seed=7) as (res, cols):
        nnan, nnull = int(nan.sum()), int(np.sum(~key.valid))
        asc = R.expected_order(cols, [(0, False)])
        assert np.array_equal(asc[n - nnan:], np.nonzero(nan)[0])                # last, in input order
        desc = R.expected_order(cols, [(0, True)])
        assert np.array_equal(desc[:nnan], np.nonzero(nan)[0]) and not key.valid[desc[n - nnull:]].any()     # first, the NULLs behind everything
        for d in DIRECTIONS:
            check(gpu_ctx, res, cols, [(0, d)])
            check(gpu_ctx, res, cols, [(0, d)], limit=nnan // 2)


def test_every_nan_pattern_is_one_window_partition_and_one_rank(gpu_ctx):
    key = nan_key()
    n = len(key)
    with built(gpu_ctx, [key], seed=7) as (res, cols):
        img, valid = R.image(key, False)
        classes = np.unique(np.stack([valid.astype(np.uint64), img]), axis=1).shape[1]         # NULL, every value, one NaN
        assert classes == 1 + len(OTHER_BITS) + 1
        order = R.expected_order(cols, [(0, False)])
        starts = np.concatenate([[True], (img[order][1:] != img[order][:-1]) | (valid[order][1:] != valid[order][:-1])])
        for part, by, want_rank, want_parts in (([0], [(0, False)], np.ones(n, dtype=np.int64), classes),
                                                ([], [(0, False)], np.cumsum(starts), 1)):
            out = gpu_ctx.window(res, part, by, [(N.WIN_DENSE_RANK,)])
            try:
                got = out.to_columns()
                assert gpu_ctx.last_window_stats()["partitions"] == want_parts
                assert np.array_equal(got[1].data, order)
                assert np.array_equal(got[3].data, want_rank)
                assert np.array_equal(got[0].data.view(np.uint64)[valid[order]], key.data.view(np.uint64)[order][valid[order]])
            finally:
                out.free()


# ---- two keys, and the sort behind the sorted-run operators --------------------------------------------------------------------

@pytest.mark.parametrize("first, second", [("block_constant", "lane_cyclic"), ("lane_cyclic", "block_constant")])
def test_two_keys_add_their_passes(gpu_ctx, first, second):
    n = N_NULL
    rng = np.random.default_rng(83)
    cols = [R.int64_key(R.layout(first, n, d=11, base=R.BASE)), nulls_over(R.layout(second, n, d=4), rng)]
    with built(gpu_ctx, cols, seed=8) as (res, cols):
        for d0, d1 in itertools.product(DIRECTIONS, repeat=2):
            assert check(gpu_ctx, res, cols, [(0, d0), (1, d1)])["radix_passes"] == 1 + (1 + 1)
            assert check(gpu_ctx, res, cols, [(1, d1), (0, d0)])["radix_passes"] == 3


def test_sorted_runs_skip_the_same_passes(gpu_ctx):
    """COUNT(DISTINCT v) per group: one sort by (group, v) through SortedRuns."""
    n = N_SKIP
    rng = np.random.default_rng(84)
    group = R.int64_key(R.one_nibble(n, 9, rng, R.BASE))
    value = R.int64_key(R.layout("lane_cyclic", n, d=13, base=R.BASE))
    with built(gpu_ctx, [group, value], seed=9) as (res, cols):
        out = gpu_ctx.group_ordered(res, [0], [(N.OSA_COUNT_DISTINCT, 1)])
        try:
            stats = gpu_ctx.last_ordered_stats()
            got = out.to_columns()
            assert stats["sorts"] == 1 and stats["groups"] == 16 and stats["rows"] == n
            assert stats["radix_passes"] == R.expected_radix_passes(cols, [(0, False), (1, False)]) == 2
            assert np.array_equal(got[0].data, np.unique(group.data))
            assert got[1].data.tolist() == [len(set(value.data[group.data == g].tolist())) for g in np.unique(group.data)]
        finally:
            out.free()


# ---- top-k ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.SELECT_CASES))
def test_top_k_select(gpu_ctx, name):
    """Rank walk, stop rule, the two half-share gates, the histogram fold and the degenerate inputs: every case is placed by
    the reference, and test_sort_patterns_cpu.py shows that it lands where it says."""
    case = R.SELECT_CASES[name]
    keycols, keys, limit = case.build()
    with built(gpu_ctx, keycols, seed=10) as (res, cols):
        stats = check(gpu_ctx, res, cols, keys, limit)      # rows, columns, and the four stats against select_model
        # c, bins, stop_cap and stopped of the intent are not reported by the device: the host file ties them to the model,
        # and check() has just tied the model's path, sorted_rows (= c) and passes to the device.  What the device does
        # report is held to the hand-written intent once more:
        for what in ("path", "select_passes"):
            if what in case.intent:
                assert stats[what] == case.intent[what], (name, stats)
