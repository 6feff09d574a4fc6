"""The host model behind test_gpu_groupby_key_patterns.py, checked without a GPU: the four hashes against literal Python-int
transcriptions, the inverses, the property every placed pattern claims, the numpy group-by reference against the C oracle, and
that the comparison the GPU test uses sees the four ways a group-by goes wrong."""
import copy

import numpy as np
import pytest

import groupby_key_pattern_reference as G
import helpers as H
from queryengine_amd import Column

EDGE_WORDS = [0, G.MASK64, 1 << 63]


def _words(n=200, seed=0):
    rng = np.random.default_rng(seed)
    return np.concatenate([np.array(EDGE_WORDS, dtype=np.uint64), rng.integers(0, 1 << 64, n, dtype=np.uint64)])


def test_hashes_match_the_python_int_transcriptions():
    a, b = _words(seed=1), _words(seed=2)[::-1].copy()
    for knull in (0, 1, 2, 3):
        one, two = G.ht_hash([a], knull), G.ht_hash([a, b], knull)
        for bits in (6, 7, 8):
            l1, l2 = G.ht_hash_lds([a], knull, bits), G.ht_hash_lds([a, b], knull, bits)
            for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
                assert l1[i] == G.ht_hash_lds_int([x], knull, bits) and l2[i] == G.ht_hash_lds_int([x, y], knull, bits)
        for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
            assert int(one[i]) == G.ht_hash_int([x], knull) and int(two[i]) == G.ht_hash_int([x, y], knull)
    for knull in (None, 0, 1, 3):
        kn = None if knull is None else np.full(len(a), knull, np.uint64)
        one, two = G.hp_hash([a], kn), G.hp_hash([a, b], kn)
        for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
            assert int(one[i]) == G.hp_hash_int([x], knull) and int(two[i]) == G.hp_hash_int([x, y], knull)
    for shift in (6, 8, 12):
        one, two = G.hp_line_bucket([a], shift), G.hp_line_bucket([a, b], shift)
        for i, (x, y) in enumerate(zip(a.tolist(), b.tolist())):
            assert one[i] == G.hp_line_bucket_int([x], shift) and two[i] == G.hp_line_bucket_int([x, y], shift)
    # partition and records-layout bucket are the top bits of the mix
    part, bucket = G.hp_group([a], 64, 8)
    for i, x in enumerate(a.tolist()):
        top = G.hp_hash_int([x]) >> 50
        assert (part[i], bucket[i]) == (top >> 8, top & 255)


def test_inverses_round_trip():
    h, later = _words(seed=3), _words(seed=4)
    for knull in (0, 1):
        k = G.ht_hash_inverse(h, knull)
        assert np.array_equal(G.ht_hash([k], knull), h) and np.array_equal(G.ht_hash_inverse(G.ht_hash([h], knull), knull), h)
        k = G.ht_hash_inverse(h, knull, later_kws=[later])
        assert np.array_equal(G.ht_hash([k, later], knull), h)
    for knull in (None, np.ones(len(h), np.uint64)):
        k = G.hp_hash_inverse(h, knull)
        assert np.array_equal(G.hp_hash([k], knull), h) and np.array_equal(G.hp_hash_inverse(G.hp_hash([h], knull), knull), h)


def test_sizes_of_the_plan_shapes_the_patterns_run_on():
    assert G.hash_words(1) == 14 and G.lds_table_bits(1) == 8 and G.lds_table_bits(2) == 8      # 256-entry LDS tables
    assert G.dense_shape(513) == ("dense_lds", 513, 0) and G.dense_shape(5001) == ("dense_key_range", 512, 10)
    assert G.ids_shape(300) == (1 << 16, 0) and G.ids_shape(4096) == (1 << 16, 9) and G.ids_shape(4097) == (1 << 16, 17)
    assert G.ids_shape(32767) == (1 << 16, 65) and G.ids_shape(32768) == (1 << 18, 65)
    assert G.hp_known_shape(160) == (256, 256) and G.hp_known_shape(300) == (256, 256) and G.hp_known_shape(100_000) == (256, 4096)
    assert G.hp_known_shape(500_000) == (512, 4096) and G.hp_known_shape(2_000_000) == (1024, 4096)
    assert G.hp_line_records(1) == 6 and G.hp_line_records(2) == 4


def _key_words(p):
    c = p.key_cols[0]
    return c.data.astype(np.int64).view(np.uint64)


def _distinct(p):
    return len(p.want[0])


@pytest.mark.parametrize("name", G.PATTERN_NAMES)
def test_pattern_has_the_property_it_claims(name):
    p = G.patterns()[name]
    c = p.claims
    kw = _key_words(p)
    n = len(p.v)
    assert n <= 70_000 and all(len(col) == n for col in p.key_cols)
    if "distinct" in c:
        assert _distinct(p) == c["distinct"]
    bits = G.lds_table_bits(p.nkeys)
    if "lds_slot" in c:
        assert set(G.ht_hash_lds([kw], 0, bits).tolist()) == {c["lds_slot"]}
        # every key in every 1024-row sub-tile (in every window of `distinct` rows): each workgroup meets them all
        d = c["distinct"]
        assert d <= 1024 and all(len(np.unique(kw[s:s + d])) == d for s in range(0, n - d, 997))
    if "hash_low16" in c:
        assert set((G.ht_hash([kw]) & np.uint64(0xFFFF)).tolist()) == {c["hash_low16"]}
    if name == "global_wrap_300":
        assert c["hash_low16"] + 300 - G.LDS_PROBE_WINDOW > G.FIRST_CAPACITY      # whatever 32 keys stay in LDS, the rest wrap
    if c.get("bits_16_18_spread"):
        h = G.ht_hash([np.unique(kw)])
        per = np.bincount(((h >> np.uint64(16)) & np.uint64(7)).astype(np.int64), minlength=8)
        assert c["distinct"] > G.GLOBAL_PROBE_LIMIT and per.max() <= 513 and per.min() >= 512
    if "id_line" in c:
        assert set((G.ht_hash([kw]) & np.uint64(0xFFFF) & ~np.uint64(7)).tolist()) == {c["id_line"]} and c["id_line"] + 8 == G.FIRST_CAPACITY
    if "id_group" in c:
        k2 = p.key_cols[1].data.astype(np.int64).view(np.uint64)
        assert set((G.ht_hash([kw, k2]) & np.uint64(0xFFFF) & ~np.uint64(3)).tolist()) == {c["id_group"]} and c["id_group"] + 4 == G.FIRST_CAPACITY
    if name == "lds_null_and_zero_share_the_key_word":
        col = p.key_cols[0]
        words = np.where(col.valid, col.data, 0)
        assert (words == 0).sum() > (~col.valid).sum() > 0 and _distinct(p) == 4
    if p.route == "key_range":
        col = p.key_cols[0]
        gp, parts = c["part_groups"], c["parts"]
        code = np.where(col.valid, col.data, len(col.dictionary)) if col.valid is not None else col.data
        used = set((code // gp).tolist())
        assert (len(col.dictionary) + gp) // gp == parts
        if name == "key_range_partition_edges":
            assert set(code.tolist()) == {e for q in range(1, parts) for e in (q * gp - 1, q * gp)}
        elif name == "key_range_partial_last_partition":
            assert used == {parts - 1} and (len(col.dictionary) + 1) % gp != 0
        elif name == "key_range_one_partition":
            assert used == {3} and len(set(code.tolist())) == gp
        else:
            assert set(code[code // gp == parts - 1].tolist()) == {len(col.dictionary)} and len(used) > 1
    if "top_bits" in c:
        top, nbits = c["top_bits"]
        h = G.hp_hash([kw])
        assert set((h >> np.uint64(64 - nbits)).tolist()) == {top}
        for parts in (64, 256) if nbits >= 8 else (64,):
            assert len(set(G.hp_group([kw], parts, 8)[0].tolist())) == 1
        if nbits >= 10:
            assert all(len(set(G.hp_group([kw], parts, 8)[0].tolist())) == 1 for parts in (512, 1024))
        if c.get("next2_spread"):
            per = np.bincount(G.hp_group([np.unique(kw)], 256, 8)[0] & 3, minlength=4)
            assert per.tolist() == [75, 75, 75, 75]
        if "line_bucket" in c:
            assert set(G.hp_line_bucket([kw], 8).tolist()) == {c["line_bucket"]} == {255}
        if "record_bucket" in c:
            assert all(set(G.hp_group([kw], parts, 8)[1].tolist()) == {255} for parts in (64, 256))
    if "tile_runs" in c:
        want_part, R = c["row_partition"], c["R"]
        assert R == G.hp_line_records(1) and n == 2 * G.SCATTER_TILE_ROWS + 17
        assert np.array_equal(G.hp_group([kw], 64, 8)[0], want_part) and np.array_equal(G.hp_group([kw], 256, 8)[0], 4 * want_part)
        seen = set()
        for t, runs in enumerate(c["tile_runs"]):
            tile = want_part[t * G.SCATTER_TILE_ROWS:(t + 1) * G.SCATTER_TILE_ROWS]
            per = np.bincount(tile, minlength=64)
            for q in range(8):
                assert per[q] == runs.get(q, 0), (t, q)
                seen.add(int(per[q]))
        assert {0, 1, R - 1, R, R + 1} <= seen
        runs0, runs1 = c["tile_runs"]
        assert 1 not in runs0 and 5 not in runs0 and runs0[0] > 0 and runs0[2] > 0 and runs0[4] > 0 and runs0[6] > 0     # empty between full
        assert runs0[0] % R != 0 and (runs0[0] + runs1[0]) % R == 0                                                      # the carry closes a line
    if c.get("last_row_group"):
        col = p.key_cols[0].data
        g = c["distinct"]
        assert np.all(np.diff(col[:g - 1]) < 0) and col[n - 1] < col[:n - 1].min() and len(np.unique(col[:n - 1])) == g - 1
        assert np.array_equal(p.want[0].data, np.sort(np.unique(col))[::-1])


@pytest.mark.parametrize("name", G.PATTERN_NAMES)
def test_reference_agrees_with_the_oracle(oracle, name):
    p = G.patterns()[name]
    rows = oracle.filter_groupby(p.cols, None, p.key_exprs, p.agg_exprs, G.AGGS, oracle.BYTECODE_COMPILER, max_groups=1 << 16)
    H._rows_equal(G.columns_to_rows(p.want), rows, p.nkeys, G.AGGS, oracle)


def _mutations(want):
    """The four ways a placed group-by goes wrong, applied to the reference's own output."""
    m = len(want[0])

    def take(idx):
        return [Column(c.type, c.data[idx], None if c.valid is None else c.valid[idx], c.dictionary) for c in want]
    dropped = take(np.delete(np.arange(m), m // 2))
    merged = take(np.delete(np.arange(m), m // 2 + 1))                     # group m/2 + 1 folded into group m/2
    merged[-5].data[m // 2] += want[-5].data[m // 2 + 1]
    merged[-4].data[m // 2] += want[-4].data[m // 2 + 1]
    idx = np.arange(m)
    idx[[m // 2, m // 2 + 1]] = idx[[m // 2 + 1, m // 2]]
    swapped = take(idx)
    moved = copy.deepcopy(list(want))                                       # one row (value 1.0) counted into the neighbouring group
    moved[-5].data[m // 2] -= 1
    moved[-5].data[m // 2 + 1] += 1
    moved[-4].data[m // 2] -= 1.0
    moved[-4].data[m // 2 + 1] += 1.0
    return {"dropped group": dropped, "merged groups": merged, "swapped pair": swapped, "row in the neighbouring group": moved}


@pytest.mark.parametrize("name", ["lds_window_overflow_33", "lds_null_and_zero_share_the_key_word", "ids_two_keys_wrap_last_group_300",
                                  "key_range_partition_edges", "hp_lines_tile_runs", "hp_device_finish_4097"])
def test_comparison_sees_what_a_wrong_group_by_does(name):
    p = G.patterns()[name]
    H.assert_group_columns_equal(copy.deepcopy(list(p.want)), p.want, p.nkeys, G.AGGS, int(G.AF.AVG), name)
    for what, bad in _mutations(p.want).items():
        with pytest.raises(AssertionError):
            H.assert_group_columns_equal(bad, p.want, p.nkeys, G.AGGS, int(G.AF.AVG), f"{name}: {what}")


def test_stats_accessor_is_bound_and_zero_before_the_first_group_by(native_lib):
    import ctypes as C
    from queryengine_amd import engine as E, native as N
    ctx = E.Context(device=-1)
    try:
        out = (C.c_int64 * 4)(7, 7, 7, 7)
        assert native_lib.qe_ctx_last_groupby_stats(ctx.handle, out) == N.OK and list(out) == [0, 0, 0, 0]
        assert native_lib.qe_ctx_last_groupby_stats(None, out) != N.OK and native_lib.qe_ctx_last_groupby_stats(ctx.handle, None) != N.OK
        assert ctx.last_groupby_stats() == {"route": "none", "abandoned": 0, "capacity": 0, "partitions": 0}
        assert len(N.GROUPBY_ROUTES) == 8
    finally:
        ctx.close()
