"""The hash equi-join at the sizes where its launch shapes change (qe_join.hip, qe_join.cpp): the trips of the
one-workgroup scans, the grid-stride loops behind the capped grids, every directory width mod 4, and the second walk of a
bucket in which other keys stand between the matches.

The expectation is tests/join_reference.py (numpy; proved equal to the host branch of ``HashJoinOperator`` in
tests/test_join_cpu.py), and EVERY output column is compared in full.  All data is seeded; every side carries a row id, a
nullable BOOLEAN, a nullable STRING, an INT32 and a DOUBLE behind its key columns, so both gather widths and both bit
gathers are in every output.  Each test asserts from the reference alone the block / row / pair count it is about: the sizes
are the boundaries of the kernels, not round numbers above them."""
import numpy as np
import pytest

from helpers import col
from join_reference import assert_join_output, expected_columns, expected_nullable, match_counts, reference_pairs
from test_gpu_join import ANTI, INNER, JOIN_NAMES, LEFT, SEMI, as_side, side_nullable
from queryengine_amd import AggregationFunction as AF
from queryengine_amd import Column, DataType
from queryengine_amd import engine as E

pytestmark = pytest.mark.gpu
D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
TAGS = ["t0", "", "täg", "t3", "t4"]
PROBE_BLOCK = 256                # rows per block of join_count_kernel / join_write_kernel
SCAN_WIDTH = 1024                # block sums per trip of the join's launch_carry_scan<u64, 1024>
ROW_GRID = 8192 * 256            # threads of the capped grids of join_build_keys_kernel, join_directory_kernel, gather_rows_kernel
GATHER_GRID = 16384 * 256        # ... of gather_rows_kernel and gather_bits_rows_kernel as the join launches them for its output columns
RADIX_SCAN_WIDTH = 1024          # counters per trip of the radix pass's launch_carry_scan<u32, 1024>: 16 per 1024 rows


def payload(rng, n, specials=True):
    """(INT64 row id, nullable BOOLEAN, nullable STRING, INT32, DOUBLE: integer valued, with NaN and -0.0 if `specials`)."""
    dbl = rng.integers(-50, 50, n).astype(np.float64)
    if specials:
        dbl = np.where(rng.random(n) < 0.05, np.array([float("nan"), -0.0])[rng.integers(0, 2, n)], dbl)
    return [Column(I64, np.arange(n, dtype=np.int64)), Column(B, rng.random(n) > 0.3, rng.random(n) > 0.2),
            Column(S, rng.integers(0, len(TAGS), n).astype(np.int32), rng.random(n) > 0.1, TAGS),
            Column(I32, rng.integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)), Column(D, dbl)]


def with_nulls(rng, data, share):
    return Column(I64, data, rng.random(len(data)) >= share)


class Sides:
    """Both sides on the device, and one hash table over the build side."""

    def __init__(self, ctx, pcols, bcols, pk, bk, kinds=("batch", "batch")):
        self.ctx, self.pcols, self.bcols, self.pk, self.bk = ctx, pcols, bcols, list(pk), list(bk)
        self.pside, self.pfree = as_side(ctx, pcols, kinds[0])
        self.bside, self.bfree = as_side(ctx, bcols, kinds[1])
        self.table = ctx.join_build(self.bside, self.bk)
        self.keyed = np.ones(len(bcols[0]), dtype=bool)
        for c in self.bk:
            if bcols[c].valid is not None:
                self.keyed &= bcols[c].valid
        assert self.table.rows == int(self.keyed.sum())
        self.probe_out = list(range(len(pk), len(pcols))) + [self.pk[0]]            # every payload type, then a key column
        self.build_out = list(range(len(bk), len(bcols))) + [self.bk[0]]

    def probe(self, jt, what="", keep=False):
        """One probe, the whole output against the reference.  -> (prow, brow, expected columns[, the result if `keep`])"""
        build_out = self.build_out if jt in (INNER, LEFT) else []
        prow, brow = reference_pairs(self.pcols, self.bcols, self.pk, self.bk, jt)
        want = expected_columns(self.pcols, self.bcols, prow, brow, self.probe_out, build_out, jt)
        res = self.table.probe(self.pside, self.pk, jt, self.probe_out, build_out)
        try:
            assert self.ctx.last_join_stats()[:3] == [self.table.rows, len(self.pcols[0]), len(prow)], (what, self.ctx.last_join_stats())
            assert res.count == len(prow), (what, res.count, len(prow))
            assert_join_output(res.to_columns(), want, brow if jt in (INNER, LEFT) else None, len(self.probe_out), what)
            nullable = expected_nullable(side_nullable(self.pside, self.pcols), side_nullable(self.bside, self.bcols), self.probe_out, build_out, jt)
            assert [bool(res.view(k).nullable) for k in range(res.ncols)] == nullable, what
        except BaseException:
            res.free()
            raise
        if keep:
            return prow, brow, want, res
        res.free()
        return prow, brow, want

    def free(self):
        self.table.free()
        for h in self.pfree + self.bfree:
            h.free()


def repeated_keys(rng, values, times):
    """values[i] times[i] times over, shuffled."""
    return rng.permutation(np.repeat(values, times))


# ---- a. the scan over the probe blocks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16_385, 262_144, 262_401])
def test_scan_of_the_block_sums_past_one_wave_and_past_one_trip(gpu_ctx, n):
    """65 blocks: a wave other than wave 0 adds the sums of the waves before it; 1024 blocks: exactly one full trip; 1026
    blocks: a second trip that starts from the carry, with a last block of one row."""
    nblocks = -(-n // PROBE_BLOCK)
    assert nblocks == {16_385: 65, 262_144: SCAN_WIDTH, 262_401: SCAN_WIDTH + 2}[n]
    rng = np.random.default_rng([61, n])
    nkeys = 400
    times = rng.integers(0, 6, nkeys)                                             # 0 .. 5 build rows per key: about 1000 rows
    present, absent = np.nonzero(times > 0)[0], np.nonzero(times == 0)[0]
    bkey = repeated_keys(rng, np.arange(nkeys, dtype=np.int64) * 1_000_003 - 7, times)
    assert 900 < len(bkey) < 1100
    bcols = [Column(I64, bkey)] + payload(rng, len(bkey))
    pkey = rng.integers(0, nkeys + 60, n) * 1_000_003 - 7                         # keys of no build row: `absent` and 400 .. 459
    valid = rng.random(n) >= 0.03
    for jt in (INNER, LEFT, SEMI, ANTI):
        # the first and the last block give pairs under every join type: a matching and an absent key in the first block,
        # and the last row (alone in its block when n = 262 401) matches unless the join keeps the rows that do not
        pkey[0], pkey[1] = present[0] * 1_000_003 - 7, absent[0] * 1_000_003 - 7
        pkey[n - 1] = (absent[1] if jt == ANTI else present[1]) * 1_000_003 - 7
        valid[[0, 1, n - 1]] = True
        pcols = [Column(I64, pkey.copy(), valid.copy())] + payload(rng, n)
        s = Sides(gpu_ctx, pcols, bcols, [0], [0], ("result", "batch") if jt == LEFT else ("batch", "batch"))
        try:
            prow, _, _ = s.probe(jt, f"{JOIN_NAMES[jt]} n={n}")
        finally:
            s.free()
        sums = np.bincount(prow // PROBE_BLOCK, minlength=nblocks)
        assert len(sums) == nblocks and sums[0] > 0 and sums[-1] > 0                # both ends contribute
        assert len(np.unique(sums[:-1])) > 8                                      # block sums differ: a wrong offset moves pairs
        if nblocks > SCAN_WIDTH:
            assert sums[:SCAN_WIDTH].sum() > 0 and sums[SCAN_WIDTH:].sum() > 0    # the second trip starts from a carry > 0
        assert not valid.all() and 0 < len(prow) != n


# ---- b. the directory -----------------------------------------------------------------------------------------------------
DIR_BITS = {16: 4, 17: 5, 32: 5, 33: 6, 100: 7, 256: 8, 257: 9, 2_000: 11, 4_096: 12, 4_097: 13, 65_536: 16, 65_537: 17}


@pytest.mark.parametrize("m", sorted(DIR_BITS))
def test_directory_of_every_width_mod_4_and_both_sides_of_a_power_of_two(gpu_ctx, m):
    """dbits = the first width with 2^dbits >= keyed rows (at least 4); the sort covers ceil(dbits / 4) digits, so dbits mod 4
    says how many hash bits below the bucket bits are sorted.  65 537 rows also take the radix pass's carry scan past one trip."""
    dbits = 4
    while (1 << dbits) < m:
        dbits += 1
    assert dbits == DIR_BITS[m]
    assert sorted({b % 4 for b in DIR_BITS.values()}) == [0, 1, 2, 3]
    if m == 65_537:
        assert 16 * -(-m // 1024) > RADIX_SCAN_WIDTH
    rng = np.random.default_rng([62, m])
    triple = max(1, m // 30)                                                      # a tenth of the rows: keys that stand three times
    ndistinct = m - 2 * triple
    values = rng.permutation(4 * m)[:ndistinct].astype(np.int64) * 2_654_435_761 - 10 ** 15
    times = np.ones(ndistinct, dtype=np.int64)
    times[:triple] = 3
    bkey = repeated_keys(rng, values, times)
    assert len(bkey) == m and len(np.unique(bkey)) == ndistinct
    bcols = [Column(I64, bkey)] + payload(rng, m)
    n = 20_000
    absent = rng.random(n) < 0.5
    pkey = np.where(absent, rng.integers(0, 4 * m, n) * 2_654_435_761 - 10 ** 15 + 1, values[rng.integers(0, ndistinct, n)])
    assert not np.isin(pkey[absent], values).any()
    pcols = [Column(I64, pkey)] + payload(rng, n)
    s = Sides(gpu_ctx, pcols, bcols, [0], [0])
    try:
        assert s.table.rows == m
        prow, brow, _ = s.probe(INNER, f"INNER m={m}")
        cnt = np.bincount(prow, minlength=n)
        assert (cnt[absent] == 0).all() and set(cnt[~absent].tolist()) == {1, 3}
        assert len(np.unique(brow)) > min(m, 5_000) // 2                          # build rows all over the table are met
        anti, _, _ = s.probe(ANTI, f"ANTI m={m}")
        assert np.array_equal(anti, np.nonzero(absent)[0])
    finally:
        s.free()


# ---- c. a build side larger than the capped grids -------------------------------------------------------------------------
@pytest.mark.parametrize("null_share", [0.03, 0.0], ids=["keyless_rows", "every_row_keyed"])
def test_build_side_past_the_grid_cap(gpu_ctx, null_share):
    """2 097 152 + 321 build rows: join_build_keys_kernel strides; more than 2^20 keyed rows: dbits >= 21, so
    join_directory_kernel strides over 2^21 + 1 entries; 3 % NULL keys: the pass that moves keyless rows behind the others
    (and the carry of the radix pass's scan) at that size.  Without NULL keys every row is keyed: gather_rows_kernel<u64> strides
    over the table's key images."""
    nb = ROW_GRID + 321
    rng = np.random.default_rng(63)
    bkey = rng.integers(0, nb // 2 + 1, nb)
    bcols = [with_nulls(rng, bkey, null_share)] + payload(rng, nb)
    keyed = nb if bcols[0].valid is None else int(bcols[0].valid.sum())
    assert nb > ROW_GRID and keyed > 2 ** 20 and (1 << 21) + 1 > ROW_GRID
    assert (keyed < nb) if null_share else (keyed > ROW_GRID)
    n = 300_000
    pkey = rng.integers(0, nb // 2 + nb // 10, n)                                 # a sixth of them beyond the build keys
    pcols = [with_nulls(rng, pkey, 0.03)] + payload(rng, n)
    s = Sides(gpu_ctx, pcols, bcols, [0], [0], ("result", "batch"))
    try:
        assert s.table.rows == keyed
        prow, brow, _ = s.probe(LEFT, f"LEFT nb={nb}")
    finally:
        s.free()
    matched = brow >= 0
    assert matched.sum() > n and (~matched).sum() > n // 10                       # most keys stand about twice; absent and NULL keys
    assert brow.max() >= ROW_GRID                                                 # build rows of the second stride are paired


# ---- d. an output larger than the gathers' capped grid --------------------------------------------------------------------
@pytest.mark.parametrize("jt", [LEFT, INNER], ids=lambda j: JOIN_NAMES[j])
def test_output_past_the_gather_cap(gpu_ctx, jt):
    """300 000 probe rows x 16 matches: more than 16384 x 256 output rows, so gather_rows_kernel (4 and 8 bytes) and
    gather_bits_rows_kernel (BOOLEAN values, validity) stride.  The INNER result then enters one more plan as a batch."""
    ctx = gpu_ctx
    rng = np.random.default_rng(64)
    nkeys, n = 200, 300_000
    values = np.arange(nkeys, dtype=np.int64) * 37 + 5
    bkey = np.concatenate([repeated_keys(rng, values, np.full(nkeys, 16)), -rng.integers(1, 1000, 300)])      # + 300 rows no probe row meets
    bkey = rng.permutation(bkey)
    bcols = [Column(I64, bkey, (bkey >= 0) | (rng.random(len(bkey)) > 0.3))] + payload(rng, len(bkey), specials=False)
    pkey = np.where(rng.random(n) < 0.05, 10 ** 9 + rng.integers(0, 1000, n), values[rng.integers(0, nkeys, n)])
    pcols = [with_nulls(rng, pkey, 0.03)] + payload(rng, n, specials=False)
    s = Sides(ctx, pcols, bcols, [0], [0], ("batch", "result"))
    try:
        prow, brow, want, res = s.probe(jt, JOIN_NAMES[jt], keep=True)
        try:
            assert len(prow) > GATHER_GRID
            cnt = match_counts(pcols, bcols, [0], [0])
            assert (cnt == 0).sum() > n // 20 and set(cnt.tolist()) == {0, 16}
            if jt == LEFT:
                assert (brow < 0).sum() == (cnt == 0).sum()
            else:
                # COUNT and SUM over the joined rows, as the next plan sees them: columns 4 and 10 are the DOUBLE payloads
                jbatch = res.as_batch()
                try:
                    assert jbatch.nrows == len(prow) and jbatch.ncols == len(want)
                    pv, bv = want[4], want[10]
                    assert pv.type == D and bv.type == D and pv.valid is None and bv.valid is None
                    exprs = [ctx.compile(col("pv", 4, D)), ctx.compile(col("bv", 10, D)), ctx.compile(col("pv", 4, D))]
                    vals, nsel = E.filter_aggregate(ctx, jbatch, None, exprs, [int(AF.COUNT), int(AF.SUM), int(AF.SUM)])
                    psum, bsum = int(pv.data.astype(np.int64).sum()), int(bv.data.astype(np.int64).sum())      # integer valued: exact
                    assert abs(psum) < 2 ** 53 and abs(bsum) < 2 ** 53 and np.abs(bv.data).sum() < 2 ** 53
                    assert nsel == len(prow) and vals == [float(len(prow)), float(bsum), float(psum)], (vals, nsel, psum, bsum)
                finally:
                    jbatch.free()
        finally:
            res.free()
    finally:
        s.free()


# ---- e. keys that share a hash, with duplicates: the second walk skips foreign entries --------------------------------------
@pytest.mark.parametrize("nkeycols", [1, 2], ids=["one_key", "two_keys"])
@pytest.mark.parametrize("bits", [0, 3])
def test_duplicate_keys_that_share_a_hash_with_other_keys(gpu_ctx, monkeypatch, bits, nkeycols):
    """QE_JOIN_HASH_BITS (read when a table is built) keeps the low `bits` bits of the hash: the directory is indexed by the
    top bits, so every entry stands in one bucket, in build-row order -- the matches of a key lie scattered among the
    entries of the other 499 keys, and join_write_kernel's walk for cnt > 1 must pick exactly them."""
    rng = np.random.default_rng([65, nkeycols])
    ndistinct, n = 500, 3_000
    times = rng.integers(1, 7, ndistinct)                                         # 1 .. 6 rows per key
    ids = repeated_keys(rng, np.arange(ndistinct), times)
    nb = len(ids)
    assert 1500 < nb < 2000
    names = ["k", "K", "k ", ""]

    def keys(i):
        """Key tuple number i: with two columns, tuples 2j and 2j + 1 share the INT64 and differ in the STRING."""
        if nkeycols == 1:
            return [Column(I64, i.astype(np.int64) * 7919 - 2_000_000)]
        return [Column(I64, (i // 2).astype(np.int64) * 7919 - 2_000_000), Column(S, ((i % 2) * 2 + (i // 2) % 2).astype(np.int32), None, names)]

    sel = rng.integers(0, ndistinct + 100, n)                                     # tuples 500 .. 599 stand in no build row
    pcols, bcols = keys(sel) + payload(rng, n), keys(ids) + payload(rng, nb)
    kc = list(range(nkeycols))
    cnt = match_counts(pcols, bcols, kc, kc)
    assert np.array_equal(cnt, np.where(sel < ndistinct, times[np.minimum(sel, ndistinct - 1)], 0))
    assert (cnt > 1).sum() > 0.7 * (cnt > 0).sum() and (cnt == 0).sum() > 100     # most matched rows walk a second time
    monkeypatch.setenv("QE_JOIN_HASH_BITS", str(bits))
    s = Sides(gpu_ctx, pcols, bcols, kc, kc)
    try:
        assert s.table.rows == nb
        for jt in (INNER, LEFT, SEMI, ANTI):
            s.probe(jt, f"{JOIN_NAMES[jt]} bits={bits}")
            longest = gpu_ctx.last_join_stats()[3]
            assert longest >= nb // 8, (longest, nb)
            if bits == 0:
                assert longest == nb, (longest, nb)                               # one hash: a row without match walks the whole table
    finally:
        s.free()
