"""The keep patterns of tests/keep_pattern_reference.py qualify for the seams they aim at, and the plain numpy reference
agrees with the C oracle -- all on the host, so that the GPU suite can trust both."""
import numpy as np
import pytest

import keep_pattern_reference as K
from helpers import assert_columns_equal

GEOS = list(K.GEOMETRIES.values())


def every_pattern(geo, n):
    """Every pattern of the GPU suite for this geometry and row count."""
    c = geo.chunk_rows
    pats = [("all",), ("none",), ("first_row",), ("last_row",), ("odd_rows",), ("even_rows",), ("lane63",), ("one_per_group",),
            ("one_per_chunk_last",)]
    for k in K.seam_counts(geo):
        pats += [("seam_head", k), ("seam_tail", k)]
    for p in (2, 3, 64, 65):
        pats += [("full_then_empty", p), ("full_then_one", p)]
    pats += [("straddle", 2 * c - 37, length) for length in (74, c, 3 * c + 1) if 2 * c - 37 + length <= n]
    pats += [("runs", 11, 40, 400), ("runs", 12, 400, 40), ("runs", 34, 5000, 50000)]
    pats += [("iid", 21, 0.03), ("iid", 22, 0.12), ("iid", 23, 0.5)]
    return pats


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: g.name)
@pytest.mark.parametrize("where", ["seam_head", "seam_tail"])
def test_seam_patterns_spill_exactly_from_ring_minus_128(geo, where):
    """Chunk 1 keeps exactly k rows and nothing else is kept; by the spill rule it spills nothing up to ring - 129 kept rows
    and at least 64 from ring - 128 on.  What stays in LDS once a chunk has spilled lies in [ring - 192, ring - 128): the
    rule never leaves a spilled chunk without an LDS-resident part, and never a full ring."""
    n = 5 * geo.chunk_rows + 129
    r = geo.ring
    resident_after_spill = set()
    for k in K.seam_counts(geo):
        mask = K.keep_mask((where, k), n, geo)
        counts = K.chunk_counts(mask, geo.chunk_rows)
        assert counts[1] == k and counts.sum() == k, (k, counts)
        spilled = K.spilled_rows(mask, geo)
        assert spilled.sum() == spilled[1] and spilled[1] % 64 == 0
        if k <= r - 129:
            assert spilled[1] == 0, (k, spilled[1])
        else:
            assert spilled[1] >= 64, (k, spilled[1])
            assert r - 192 <= k - spilled[1] < r - 128, (k, spilled[1])
            resident_after_spill.add(int(k - spilled[1]))
    # both ends of the LDS-resident part of a spilled chunk are reached: the smallest by the first spill of a chunk that
    # fills whole groups, the largest (ring - 129) where the threshold is crossed by 127 rows in the chunk's last groups
    assert r - 192 in resident_after_spill
    if where == "seam_tail":
        assert r - 129 in resident_after_spill


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: g.name)
def test_ring_has_one_spare_entry_under_the_spill_rule(geo):
    """After its spills a chunk holds at most ring - 129 rows in LDS and a load group adds at most 128: the ring never holds
    more than ring - 1 rows.  A threshold of ring - 127 would fill the ring to the last entry and still lose nothing (the same
    rows, only spilled one group later); ring - 126 is the first threshold under which a row that has not been spilled is
    overwritten, and the pattern that shows it is ring + 1 rows kept at the END of a chunk (1 row, then two full groups)."""
    n = 5 * geo.chunk_rows + 129
    r = geo.ring
    high = {128: 0, 127: 0, 126: 0}
    for where in ("seam_head", "seam_tail"):
        for k in K.seam_counts(geo):
            mask = K.keep_mask((where, k), n, geo)
            for slack in high:
                high[slack] = max(high[slack], int(K.spill_model(mask, geo, slack)[1].max()))
    assert high == {128: r - 1, 127: r, 126: r + 1}
    assert K.spill_model(K.keep_mask(("seam_tail", r + 1), n, geo), geo, 126)[1].max() == r + 1


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: g.name)
def test_full_and_empty_chunks_have_exact_counts(geo):
    c = geo.chunk_rows
    for n in (64 * c + 1, 130 * c + 7):
        last = n - (n - 1) // c * c          # rows of the ragged last chunk
        for p in (2, 3, 64, 65):
            full = np.arange(-(-n // c)) % p == 1
            counts = K.chunk_counts(K.keep_mask(("full_then_empty", p), n, geo), c)
            assert np.array_equal(counts[:-1], np.where(full, c, 0)[:-1]) and counts[-1] in (0, last)
            assert (counts == c).sum() >= 1
            counts = K.chunk_counts(K.keep_mask(("full_then_one", p), n, geo), c)
            assert np.array_equal(counts[:-1], np.where(full, c, 1)[:-1]) and counts[-1] in (1, last)
        # full chunks spill (chunk - ring is far past the threshold), the one-row chunks next to them never do
        spilled = K.spilled_rows(K.keep_mask(("full_then_one", 3), n, geo), geo)
        counts = K.chunk_counts(K.keep_mask(("full_then_one", 3), n, geo), c)
        assert (spilled[counts == c] > 0).all() and (spilled[counts == 1] == 0).all()
    # the same patterns counted in dense tiles
    t = geo.tile_rows
    counts = K.chunk_counts(K.keep_mask(("full_then_one", 2), 64 * t + 1, geo, unit=t), t)
    assert set(counts[:-1]) == {1, t} and counts[-1] == 1


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: g.name)
def test_straddle_starts_on_an_odd_row_and_crosses_chunks(geo):
    c = geo.chunk_rows
    n = 5 * c + 129
    for length in (74, c, 3 * c + 1):
        mask = K.keep_mask(("straddle", 2 * c - 37, length), n, geo)
        first = int(np.argmax(mask))
        assert first % 2 == 1 and first == 2 * c - 37 and mask.sum() == length
        counts = K.chunk_counts(mask, c)
        assert counts[1] == 37 and counts[2] == min(c, length - 37)


def test_lane_patterns_populate_the_intended_ballots():
    """A lane holds rows 2l and 2l + 1 of a 128-row load group; the ranks come from one ballot per parity."""
    geo = K.GEOMETRIES["small"]
    n = 5 * geo.chunk_rows + 129
    full = n // 128

    def ballots(name):
        m = K.keep_mask((name,), n, geo)[:full * 128].reshape(full, 64, 2)
        return m[:, :, 0], m[:, :, 1]          # per group: [lane] of the even rows, of the odd rows

    b0, b1 = ballots("odd_rows")
    assert not b0.any() and b1.all()
    b0, b1 = ballots("even_rows")
    assert b0.all() and not b1.any()
    b0, b1 = ballots("lane63")
    assert b0[:, 63].all() and b1[:, 63].all() and not b0[:, :63].any() and not b1[:, :63].any()
    b0, b1 = ballots("one_per_group")
    assert ((b0.sum(axis=1) + b1.sum(axis=1)) == 1).all()
    g = np.arange(full)
    assert np.array_equal(b0.sum(axis=1), (g % 2 == 0).astype(int))      # the row's parity alternates from group to group
    lanes = np.argmax(b0 | b1, axis=1)
    assert np.array_equal(lanes, (g % 128) // 2)                         # .. and it visits every lane
    counts = K.chunk_counts(K.keep_mask(("one_per_chunk_last",), n, geo), geo.chunk_rows)
    assert (counts[:-1] == 1).all() and counts[-1] == 0
    assert K.keep_mask(("last_row",), n, geo).nonzero()[0].tolist() == [n - 1] and n % geo.sub_rows != 0


@pytest.mark.parametrize("geo", GEOS, ids=lambda g: g.name)
def test_long_runs_fill_and_empty_whole_chunks_at_the_gpu_row_counts(geo):
    n = 65 * geo.chunk_rows + geo.sub_rows - 1
    counts = K.chunk_counts(K.keep_mask(("runs", 34, 5000, 50000), n, geo), geo.chunk_rows)
    assert (counts == 0).any() and (counts >= min(geo.chunk_rows, 4096)).any() and counts.sum() > 0
    counts = K.chunk_counts(K.keep_mask(("runs", 12, 400, 40), n, geo), geo.chunk_rows)
    assert (K.spilled_rows(K.keep_mask(("runs", 12, 400, 40), n, geo), geo)[:-1] > 0).all() and (counts < geo.chunk_rows).any()


def test_clustered_runs_have_their_mean_lengths():
    geo = K.GEOMETRIES["small"]
    n = 400_000
    for seed, mk, md in ((11, 40, 400), (12, 400, 40), (34, 5000, 50000)):
        mask = K.keep_mask(("runs", seed, mk, md), n, geo)
        edges = np.flatnonzero(np.diff(mask.astype(np.int8)))
        lens = np.diff(edges)
        keep_runs = lens[0::2] if mask[edges[0] + 1] else lens[1::2]
        if len(keep_runs) >= 100:              # enough runs for their mean to mean something (sd of the mean <= 10 %)
            assert 0.7 * mk < keep_runs.mean() < 1.3 * mk
            assert 0.7 * mk / (mk + md) < mask.mean() < 1.3 * mk / (mk + md)
        else:                                  # the long runs: whole chunks of the small geometry kept, and whole chunks dropped
            counts = K.chunk_counts(mask, geo.chunk_rows)
            assert (counts == geo.chunk_rows).any() and (counts == 0).any()


@pytest.mark.parametrize("shape", K.SHAPES)
def test_numpy_reference_equals_the_c_oracle(oracle, shape):
    """expected() (col[mask], numpy `+`) against oracle.filter_project (BYTECODE_COMPILER) for every pattern: the two
    references of the GPU suites agree, and the columns build_case makes keep exactly the mask they were given."""
    geo = K.GEOMETRIES["small"]
    n = 5 * 1024 + 129
    for tag, pattern in enumerate(every_pattern(geo, n)):
        mask = K.keep_mask(pattern, n, geo)
        case = K.build_case(shape, n, mask, tag)
        assert np.array_equal(K.filter_mask(case), mask), pattern
        want = K.expected(case.columns, mask, case.spec)
        got = oracle.filter_project(case.columns, case.filter, case.projections, oracle.BYTECODE_COMPILER)
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert_columns_equal(w, g, f"{shape} {K.pattern_id(pattern)} projection {j}")
    # another literal over the same data keeps the same rows
    mask = K.keep_mask(("runs", 11, 40, 400), n, geo)
    case = K.build_case(shape, n, mask, 9, literal=2)
    assert np.array_equal(K.filter_mask(case, 2), mask)
    for g, w in zip(oracle.filter_project(case.columns, case.filter, case.projections, oracle.BYTECODE_COMPILER),
                    K.expected(case.columns, mask, case.spec)):
        assert_columns_equal(w, g, f"{shape} literal 2")


def test_mixed_shape_has_null_filter_rows_next_to_kept_rows():
    geo = K.GEOMETRIES["small"]
    n = 5 * 1024 + 129
    for pattern in (("seam_head", 127), ("runs", 11, 40, 400), ("odd_rows",), ("full_then_one", 2)):
        mask = K.keep_mask(pattern, n, geo)
        k = K.build_case("mixed", n, mask, 1).columns[0]
        null = ~k.valid
        assert null.any() and not (null & mask).any() and (k.data[null] == 0).all()      # a NULL over a value that would pass
        assert (null[1:] & mask[:-1]).any() or (null[:-1] & mask[1:]).any()


@pytest.mark.parametrize("shape", K.SHAPES)
def test_row_ids_of_two_tags_never_collide(shape):
    geo = K.GEOMETRIES["small"]
    n = 5 * 1024 + 129
    mask = K.keep_mask(("all",), n, geo)
    ids = []
    for tag in (0, 1, 2, 255):
        case = K.build_case(shape, n, mask, tag)
        rid = case.columns[5 if shape == "mixed" else 1].data
        assert np.array_equal(rid >> 40, np.full(n, tag)) and np.array_equal(rid & ((1 << 40) - 1), np.arange(n))
        ids.append(rid)
    assert len(np.unique(np.concatenate(ids))) == 4 * n


def test_geometry_table():
    rows = {g.name: (g.tuning()[:5], g.sub_rows, g.chunk_rows, g.ring) for g in GEOS}
    assert rows == {"default": ([0, 0, 0, 0, 0], 1024, 16384, 256), "wide": ([256, 16, 0, 0, 20004], 2048, 8192, 512),
                    "mid": ([128, 8, 0, 0, 20008], 1024, 8192, 512), "small": ([256, 2, 0, 0, 4], 256, 1024, 256),
                    "small512": ([256, 2, 0, 0, 20004], 256, 1024, 512)}
    assert K.GEOMETRIES["default"].tile_rows == 4096 and K.GEOMETRIES["small"].tile_rows == 1024
    assert K.GEOMETRIES["small"].tuning(K.RING_BITS, 4, 3) == [256, 2, 0, 0, 4, K.RING_BITS, 4, 300]
    assert max(K.row_counts(K.GEOMETRIES["default"])) == 130 * 16384 + 7 and max(K.row_counts(K.GEOMETRIES["small"])) == 133_127
    assert K.fl_ring("one", K.GEOMETRIES["small"]) == 512 and K.fl_ring("mixed", K.GEOMETRIES["small"]) == 256
    assert K.GEOMETRIES["default"].dense_tile_rows(K.ROW_BYTES["one"]) == 4096
    assert K.GEOMETRIES["default"].dense_tile_rows(K.ROW_BYTES["mixed"]) == 2048
