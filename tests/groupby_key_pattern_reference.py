"""GROUP BY under PLACED keys: a host model of where the group-by's hashes put a key, the inverses that turn a wanted place
into a key, the table and partition sizes of a plan shape, a plain group-by reference, and the pattern builders whose keys
fill a probe window, wrap a table's end, exhaust a probe limit, overflow a partition or sit on a threshold -- none of which
random keys under a good hash ever do.  numpy only: no GPU, no native library.

The hashes are transcriptions of the generated device code (qe_codegen.cpp): qe_ht_hash (global table and id table),
qe_ht_hash_lds (a workgroup's LDS table), qe_hp_grp (partition and home bucket of the hash-partitioned form) and the 32-bit
fold that homes a record in the lines layout.  INT64 keys: the key word IS the value, so all 64 bits are ours.  The two 64-bit
hashes are bijections of one key word (odd multiplies, xor-shifts) and are inverted; the two 32-bit folds are searched over
the hash bits a placement leaves free.

Every pattern is a `Pattern`: the columns, the expected result columns, and `stats`: what qe_ctx_last_groupby_stats must
report on the 1st, 2nd and 3rd execution of the plan on a fresh context of the pattern's route."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from queryengine_amd import AggregationFunction as AF
from queryengine_amd import Column, ColumnExpression, DataType

D, I64, I32, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.STRING
U64, U32 = np.uint64, np.uint32
MASK64 = (1 << 64) - 1

GOLDEN, HT_SEED, M1, M2 = 0x9E3779B97F4A7C15, 0x632BE59BD9B4E019, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
GOLDEN32, LDS_NULL_MUL = 0x9E3779B1, 0x85EBCA6B
M1_INV, M2_INV = pow(M1, -1, 1 << 64), pow(M2, -1, 1 << 64)
GOLDEN32_INV = pow(GOLDEN32, -1, 1 << 32)

AGGS = [int(AF.COUNT), int(AF.SUM), int(AF.MIN), int(AF.MAX), int(AF.AVG)]      # over one integer-valued DOUBLE column v
NAGG = len(AGGS)

# debug bits of qe_options.tuning[5]
GLOBAL_ATOMICS_HASHED, FORCE_HP, HP_HEADER_RECORDS, FINISH_ON_DEVICE = 131072, 8388608, 33554432, 67108864

LDS_PROBE_WINDOW, GLOBAL_PROBE_LIMIT, FIRST_CAPACITY = 32, 4096, 1 << 16
HP_FIRST_PARTS, HP_FIRST_SHIFT = 64, 8          # a forced first execution: 64 partitions x 256 buckets
SCATTER_TILE_ROWS = 4096                        # hash-partitioned scatter: 8 waves x 4 load groups x 128 rows


def _u64(x) -> np.ndarray:
    return np.atleast_1d(np.asarray(x)).astype(U64)


def _mul(a: np.ndarray, c: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return a * U64(c)


# ---- the four hashes ----------------------------------------------------------------------------------------------------------
def ht_hash(kws: Sequence, knull=0) -> np.ndarray:
    """qe_ht_hash: the slot in the global table (`& mask`) and in the id table (`& mask & ~7`, two keys and more `& ~3`)."""
    kws = [_u64(k) for k in kws]
    h = _mul(np.broadcast_to(_u64(knull), kws[0].shape).copy(), GOLDEN) + U64(HT_SEED)
    for kw in kws:
        h = _mul(h ^ kw, M1)
        h = h ^ (h >> U64(29))
    h = _mul(h, M2)
    return h ^ (h >> U64(32))


def ht_hash_inverse(h, knull=0, later_kws: Sequence = ()) -> np.ndarray:
    """The FIRST key word whose qe_ht_hash (followed by the key words `later_kws`, under `knull`) is h."""
    h = _u64(h)
    h = h ^ (h >> U64(32))
    h = _mul(h, M2_INV)
    for kw in list(later_kws)[::-1] + [None]:
        h = h ^ (h >> U64(29)) ^ (h >> U64(58))
        h = _mul(h, M1_INV)
        if kw is not None:
            h = h ^ _u64(kw)
    return h ^ (_mul(np.broadcast_to(_u64(knull), h.shape).copy(), GOLDEN) + U64(HT_SEED))


def ht_hash_lds(kws: Sequence, knull=0, bits: int = 7) -> np.ndarray:
    """qe_ht_hash_lds: the home slot in a workgroup's LDS table of 2^bits entries."""
    kws = [_u64(k) for k in kws]
    with np.errstate(over="ignore"):
        k = np.broadcast_to(_u64(knull), kws[0].shape).astype(U32) * U32(LDS_NULL_MUL)
        for kw in kws:
            k = ((k << U32(5)) | (k >> U32(27))) ^ kw.astype(U32) ^ (kw >> U64(32)).astype(U32)
        return ((k * U32(GOLDEN32)) >> U32(32 - bits)).astype(np.int64)


def hp_hash(kws: Sequence, knull=None) -> np.ndarray:
    """The 64-bit mix of qe_hp_grp (splitmix64's finaliser over the folded key words): its TOP bits are the partition and,
    in the records layout, below them the home bucket.  `knull`: the null bits of a plan whose keys are nullable."""
    kws = [_u64(k) for k in kws]
    h = kws[0]
    for kw in kws[1:]:
        h = _mul(h, GOLDEN) + kw
    if knull is not None:
        h = h ^ (_u64(knull) << U64(57))
    h = _mul(h ^ (h >> U64(30)), M1)
    h = _mul(h ^ (h >> U64(27)), M2)
    return h ^ (h >> U64(31))


def hp_hash_inverse(h, knull=None) -> np.ndarray:
    """The one key word whose qe_hp_grp mix is h."""
    h = _u64(h)
    h = h ^ (h >> U64(31)) ^ (h >> U64(62))
    h = _mul(h, M2_INV)
    h = h ^ (h >> U64(27)) ^ (h >> U64(54))
    h = _mul(h, M1_INV)
    h = h ^ (h >> U64(30)) ^ (h >> U64(60))
    return h if knull is None else h ^ (_u64(knull) << U64(57))


def hp_group(kws: Sequence, parts: int, shift: int, knull=None) -> Tuple[np.ndarray, np.ndarray]:
    """(partition, home bucket of the records layout) = the top log2(parts) + shift bits of the mix."""
    pbits = (parts - 1).bit_length()
    grp = (hp_hash(kws, knull) >> U64(64 - pbits - shift)).astype(np.int64)
    return grp >> shift, grp & ((1 << shift) - 1)


def hp_line_bucket(words: Sequence, shift: int) -> np.ndarray:
    """Home bucket of a record in the LINES layout: the record's key words (then the null bits, where keys are nullable)
    folded to 32 bits, one multiply, the top `shift` bits."""
    with np.errstate(over="ignore"):
        hb = np.zeros(_u64(words[0]).shape, U32)
        for w in words:
            w = _u64(w)
            lo, hi = w.astype(U32), (w >> U64(32)).astype(U32)
            hb = ((hb << U32(5)) | (hb >> U32(27))) ^ lo ^ ((hi << U32(13)) | (hi >> U32(19)))
        hb = hb ^ (hb >> U32(16))
        hb = hb * U32(GOLDEN32)
        return (hb >> U32(32 - shift)).astype(np.int64)


# ---- literal Python-int transcriptions (mod 2^64), what the CPU test checks the array forms against ---------------------------
def ht_hash_int(kws: Sequence[int], knull: int = 0) -> int:
    h = (knull * GOLDEN + HT_SEED) & MASK64
    for kw in kws:
        h = ((h ^ kw) * M1) & MASK64
        h ^= h >> 29
    h = (h * M2) & MASK64
    return h ^ (h >> 32)


def ht_hash_lds_int(kws: Sequence[int], knull: int = 0, bits: int = 7) -> int:
    k = (knull & 0xFFFFFFFF) * LDS_NULL_MUL & 0xFFFFFFFF
    for kw in kws:
        k = (((k << 5) | (k >> 27)) & 0xFFFFFFFF) ^ (kw & 0xFFFFFFFF) ^ (kw >> 32)
    return ((k * GOLDEN32) & 0xFFFFFFFF) >> (32 - bits)


def hp_hash_int(kws: Sequence[int], knull: Optional[int] = None) -> int:
    h = kws[0]
    for kw in kws[1:]:
        h = (h * GOLDEN + kw) & MASK64
    if knull is not None:
        h ^= (knull << 57) & MASK64
    h ^= h >> 30
    h = (h * M1) & MASK64
    h ^= h >> 27
    h = (h * M2) & MASK64
    return h ^ (h >> 31)


def hp_line_bucket_int(words: Sequence[int], shift: int) -> int:
    hb = 0
    for w in words:
        lo, hi = w & 0xFFFFFFFF, w >> 32
        hb = (((hb << 5) | (hb >> 27)) & 0xFFFFFFFF) ^ lo ^ (((hi << 13) | (hi >> 19)) & 0xFFFFFFFF)
    hb ^= hb >> 16
    hb = (hb * GOLDEN32) & 0xFFFFFFFF
    return hb >> (32 - shift)


# ---- table and partition sizes of a plan shape --------------------------------------------------------------------------------
def hash_words(nkeys: int, nagg: int = NAGG) -> int:
    return 3 + nkeys + 2 * nagg                  # {state, null bits, key words.., first row, (count, acc)..}


def lds_table_bits(nkeys: int, nagg: int = NAGG) -> int:
    """hashed_prelude: the largest power of two of entries with 2 * entries * entry bytes <= 48 KiB."""
    bits = 0
    while (2 << bits) * hash_words(nkeys, nagg) * 8 <= 48 * 1024:
        bits += 1
    return bits


def dense_shape(ngroups: int, nagg: int = NAGG) -> Tuple[str, int, int]:
    """(route, capacity, partitions) of a dense plan over `ngroups` group ids (domain + its NULL code): one LDS table up to
    144 KiB, else the key-range partitions of the largest power of two of groups whose table fits 80 KiB."""
    words = 1 + 2 * nagg
    if ngroups * words * 8 <= 144 * 1024:
        return "dense_lds", ngroups, 0
    shift = 0
    while shift < 12 and (2 << shift) * words * 8 <= 80 * 1024:
        shift += 1
    return "dense_key_range", 1 << shift, (ngroups + (1 << shift) - 1) >> shift


def ids_shape(distinct: int, nagg: int = NAGG) -> Tuple[int, int]:
    """(id table entries, partitions of the dense pass over the ids) of run_groupby_ids on a plan's first id build: the
    table starts at 65 536 entries and grows x4 while the ids reach half of it; the id domain is the next power of two."""
    cap = FIRST_CAPACITY
    while distinct > (cap - 1) >> 1:
        cap *= 4
    dom = 2
    while dom < distinct:
        dom *= 2
    return cap, dense_shape(dom + 1, nagg)[2]


def hp_known_shape(keys_seen: int, max_shift: int = 12, fill: int = 16) -> Tuple[int, int]:
    """(partitions, buckets per partition) that run_groupby_hashed_route sizes from the key count of an earlier execution."""
    parts = 256 if keys_seen * 10 <= (256 << max_shift) * 3 else 512 if keys_seen * 2 <= (512 << max_shift) else 1024
    shift = 8
    while shift < max_shift and (parts << shift) < keys_seen * fill:
        shift += 1
    return parts, 1 << shift


def hp_line_records(nkey_words: int, nvals: int = 1) -> int:
    """R: records per 128-byte line {R x (value and key words), R x 32-bit row id, R x flag byte}."""
    return 128 // (8 * (nvals + nkey_words) + 5)


# ---- the group-by reference -----------------------------------------------------------------------------------------------------
def values_for(n: int) -> np.ndarray:
    """Integer-valued doubles, a function of the row: every sum of them is exact in any order."""
    i = np.arange(n, dtype=np.int64)
    return ((i * 7919 + 13) % 2001 - 1000).astype(np.float64)


def groupby_reference(key_cols: Sequence[Column], v: np.ndarray) -> List[Column]:
    """SELECT keys.., COUNT(v), SUM(v), MIN(v), MAX(v), AVG(v) GROUP BY keys..: the groups in order of first appearance, NULL a
    key value of its own; exact on integer-valued v."""
    n = len(v)
    words = []
    for c in key_cols:
        ok = c.valid if c.valid is not None else np.ones(n, bool)
        words += [np.where(ok, c.data.astype(np.int64), 0), ok]
    order = np.lexsort(words[::-1]) if n else np.zeros(0, np.int64)      # stable: equal tuples keep their row order
    change = np.ones(n, bool)
    if n:
        same = np.ones(n - 1, bool)
        for w in words:
            same &= w[order][1:] == w[order][:-1]
        change[1:] = ~same
    starts = np.nonzero(change)[0]
    first_rows = order[starts] if n else starts
    by_first = np.argsort(first_rows, kind="stable")
    sv = v[order]
    cnt = np.diff(np.append(starts, n)).astype(np.float64)
    if n:
        ssum, smin, smax = np.add.reduceat(sv, starts), np.minimum.reduceat(sv, starts), np.maximum.reduceat(sv, starts)
    else:
        ssum = smin = smax = np.zeros(0)
    rows = first_rows[by_first]
    out = [Column(c.type, c.data[rows], None if c.valid is None else c.valid[rows], c.dictionary) for c in key_cols]
    for a in (cnt, ssum, smin, smax, ssum / np.maximum(cnt, 1)):
        out.append(Column(D, a[by_first], None))
    return out


def columns_to_rows(cols: Sequence[Column]) -> list:
    """Result columns as the oracle's rows [key values.., aggregate values..] (None = NULL, STRING keys as strings)."""
    lists = []
    for c in cols:
        vals = c.data.tolist()
        if c.dictionary is not None:
            vals = [c.dictionary[x] for x in vals]
        if c.valid is not None:
            vals = [x if ok else None for x, ok in zip(vals, c.valid.tolist())]
        lists.append(vals)
    return [list(r) for r in zip(*lists)]


# ---- patterns ---------------------------------------------------------------------------------------------------------------------
def stats(route: str, abandoned: int, capacity: int, partitions: int) -> Dict:
    return {"route": route, "abandoned": abandoned, "capacity": capacity, "partitions": partitions}


@dataclass
class Pattern:
    name: str
    route: str                       # the context (tuning word, schema) the pattern runs on: a key of ROUTE_WORDS
    key_cols: List[Column]
    v: np.ndarray
    stats: List[Dict]                # of executions 1, 2, 3
    claims: Dict = field(default_factory=dict)      # what the CPU test checks about the placement
    _want: Optional[List[Column]] = None

    @property
    def cols(self) -> List[Column]:
        return list(self.key_cols) + [Column(D, self.v, None)]

    @property
    def key_exprs(self):
        return [ColumnExpression(f"k{i}", i, c.type) for i, c in enumerate(self.key_cols)]

    @property
    def agg_exprs(self):
        return [ColumnExpression("v", len(self.key_cols), D)] * NAGG

    @property
    def want(self) -> List[Column]:
        if self._want is None:
            self._want = groupby_reference(self.key_cols, self.v)
        return self._want

    @property
    def nkeys(self) -> int:
        return len(self.key_cols)


# route -> tuning[5]; one schema and one aggregate list per route, so every route compiles once
ROUTE_WORDS = {
    "lds": 0, "lds_spill": GLOBAL_ATOMICS_HASHED, "lds_nullable": 0,
    "global": GLOBAL_ATOMICS_HASHED,
    "ids": 0, "ids_two_keys": 0,
    "key_range": 0,
    "hp_lines": FORCE_HP, "hp_records": FORCE_HP | HP_HEADER_RECORDS,
    "hp_device": FORCE_HP | FINISH_ON_DEVICE,
}


def _as_i64(words: np.ndarray) -> np.ndarray:
    return np.asarray(words, dtype=U64).view(np.int64)


def _cyclic(keys: np.ndarray, n: int) -> np.ndarray:
    """Row i holds key i mod len(keys): every window of len(keys) rows holds every key."""
    return keys[np.arange(n) % len(keys)]


def _pattern(name, route, keys_i64, n, st, claims=None, extra_cols=(), valid=None) -> Pattern:
    col = Column(I64, keys_i64, valid)
    return Pattern(name, route, [col] + list(extra_cols), values_for(n), st, claims or {})


def keys_with_lds_slot(slot: int, count: int, bits: int, seed: int) -> np.ndarray:
    """`count` distinct INT64 key words homed at `slot` of an LDS table of 2^bits entries: the 32-bit multiply is inverted for the
    fold lo ^ hi, the high half is free."""
    rng = np.random.default_rng(seed)
    free = rng.choice(1 << (32 - bits), count, replace=False).astype(np.uint64)
    product = (U64(slot) << U64(32 - bits)) | free
    fold = _mul(product, GOLDEN32_INV) & U64(0xFFFFFFFF)
    hi = rng.integers(0, 1 << 32, count, dtype=np.uint64)
    return (hi << U64(32)) | (fold ^ hi)


def keys_with_hash_bits(low: np.ndarray, low_bits: int, seed: int) -> np.ndarray:
    """One key word per entry of `low`: its qe_ht_hash ends in the `low_bits` bits low[i]; the bits above are drawn."""
    rng = np.random.default_rng(seed)
    free = rng.choice(1 << 40, len(low), replace=False).astype(np.uint64)          # distinct hashes => distinct keys
    return ht_hash_inverse((free << U64(low_bits)) | _u64(low))


def keys_with_hash_low_bits_and_lds_slot(low: int, low_bits: int, count: int, seed: int, lds_slot: int, lds_bits: int) -> np.ndarray:
    """`count` distinct key words whose qe_ht_hash ends in the `low_bits` bits `low` AND whose LDS home slot is `lds_slot`: a
    search over the free hash bits (one candidate in 2^lds_bits hits)."""
    rng = np.random.default_rng(seed)
    out = np.zeros(0, U64)
    while len(out) < count:
        free = rng.integers(0, 1 << (64 - low_bits), (count << lds_bits) * 2 + 64, dtype=np.uint64)
        kw = ht_hash_inverse((free << U64(low_bits)) | U64(low))
        out = np.unique(np.concatenate([out, kw[ht_hash_lds([kw], 0, lds_bits) == lds_slot]]))
    return rng.permutation(out)[:count]


def keys_with_hp_top_bits(top: int, top_bits: int, count: int, seed: int, line_bucket: Optional[int] = None, shift: int = 8,
                          next_bits: Optional[np.ndarray] = None, nnext: int = 0) -> np.ndarray:
    """`count` distinct key words whose qe_hp_grp mix starts with the `top_bits` bits `top` (then the `nnext` bits
    next_bits[i]) and -- a search over the free bits -- whose lines-layout home bucket is `line_bucket`."""
    rng = np.random.default_rng(seed)
    out: List[np.ndarray] = []
    have = 0
    free_bits = 64 - top_bits - nnext
    while have < count:
        need = count - have
        m = need * ((1 << shift) if line_bucket is not None else 1) * 2 + 64
        free = rng.integers(0, 1 << free_bits, m, dtype=np.uint64)
        nb = np.zeros(m, U64) if nnext == 0 else np.resize(next_bits[have:].astype(U64), m)
        h = (U64(top) << U64(64 - top_bits)) | (nb << U64(free_bits)) | free
        kw = hp_hash_inverse(h)
        if line_bucket is not None:
            assert nnext == 0
            kw = kw[hp_line_bucket([kw], shift) == line_bucket]
        kw = kw[:need]
        out.append(kw)
        have += len(kw)
    keys = np.concatenate(out)
    assert len(np.unique(keys)) == count
    return keys


def build_patterns() -> Dict[str, Pattern]:
    pats: Dict[str, Pattern] = {}

    def add(p: Pattern):
        assert p.name not in pats and p.route in ROUTE_WORDS and len(p.v) <= 70_000
        pats[p.name] = p

    bits = lds_table_bits(1)
    nslots = 1 << bits
    n_small = 3 * 4096 + 17                        # more than one workgroup tile, a ragged tail
    hashed0 = stats("hashed", 0, FIRST_CAPACITY, 0)

    # ---- workgroup LDS tables (probe window 32) ----
    k32 = keys_with_lds_slot(5, 32, bits, 1)
    add(_pattern("lds_window_full_32", "lds", _as_i64(_cyclic(k32, n_small)), n_small, [hashed0] * 3,
                 {"lds_slot": 5, "distinct": 32}))
    k33 = keys_with_lds_slot(5, 33, bits, 2)
    ids33 = stats("dense_ids", 0, *ids_shape(33))
    add(_pattern("lds_window_overflow_33", "lds", _as_i64(_cyclic(k33, n_small)), n_small,
                 [dict(ids33, abandoned=1), ids33, ids33], {"lds_slot": 5, "distinct": 33}))
    add(_pattern("lds_window_overflow_33_spills_to_global", "lds_spill", _as_i64(_cyclic(k33, n_small)), n_small, [hashed0] * 3,
                 {"lds_slot": 5, "distinct": 33}))
    k20 = keys_with_lds_slot(nslots - 1, 20, bits, 3)
    add(_pattern("lds_wrap_last_slot_20", "lds", _as_i64(_cyclic(k20, n_small)), n_small, [hashed0] * 3,
                 {"lds_slot": nslots - 1, "distinct": 20}))
    kn = np.array([0, 0, -1, np.iinfo(np.int64).min], dtype=np.int64)
    vn = np.array([False, True, True, True])
    add(_pattern("lds_null_and_zero_share_the_key_word", "lds_nullable", _cyclic(kn, n_small), n_small, [hashed0] * 3,
                 {"distinct": 4}, valid=_cyclic(vn, n_small)))

    # ---- global table (global atomics kept: first capacity 65 536, then x8) ----
    low = FIRST_CAPACITY - 3
    kg = keys_with_hash_low_bits_and_lds_slot(low, 16, 300, 4, 9, bits)
    add(_pattern("global_wrap_300", "global", _as_i64(_cyclic(kg, n_small)), n_small, [hashed0] * 3,
                 {"hash_low16": low, "lds_slot": 9, "distinct": 300}))
    nprobe = GLOBAL_PROBE_LIMIT + 1
    kp = keys_with_hash_bits(77 + ((np.arange(nprobe) % 8) << 16), 19, 5)
    big = stats("hashed", 0, FIRST_CAPACITY * 8, 0)
    add(_pattern("global_probe_limit_4097", "global", _as_i64(_cyclic(kp, 3 * nprobe + 5)), 3 * nprobe + 5,
                 [dict(big, abandoned=1), big, big], {"hash_low16": 77, "distinct": nprobe, "bits_16_18_spread": True}))
    rng = np.random.default_rng(6)
    half = rng.permutation(np.arange(1, 1 << 16, dtype=np.int64))[:1 << 15] * 1_000_003
    add(_pattern("global_half_full_32767", "global", _cyclic(half[:32767], 40_000), 40_000, [hashed0] * 3, {"distinct": 32767}))
    add(_pattern("global_half_full_32768", "global", _cyclic(half, 40_000), 40_000, [dict(big, abandoned=1), big, big],
                 {"distinct": 32768}))

    # ---- dense ids (qe_ht_build); the first execution of a plan finds out in its LDS tables (code 4) ----
    def ids_stats(distinct, first_extra=0):
        cap, parts = ids_shape(distinct)
        st = stats("dense_ids", 0, cap, parts)
        return [dict(st, abandoned=1 + first_extra), st, st]

    ki = keys_with_hash_bits(FIRST_CAPACITY - 8 + np.arange(300) % 8, 16, 7)     # anywhere in the last line: `& ~7` starts them all at its head
    add(_pattern("ids_wrap_last_line_300", "ids", _as_i64(_cyclic(ki, n_small)), n_small, ids_stats(300),
                 {"id_line": FIRST_CAPACITY - 8, "distinct": 300}))
    for d in (32767, 32768):
        add(_pattern(f"ids_first_table_{d}", "ids", _cyclic(half[:d], 40_000), 40_000, ids_stats(d, 1 if d == 32768 else 0),
                     {"distinct": d}))
    for d in (4096, 4097):
        add(_pattern(f"ids_domain_{d}", "ids", _cyclic(half[:d], 3 * d + 11), 3 * d + 11, ids_stats(d), {"distinct": d}))
    # two keys (INT64, INT32): the INT64 word is solved for the wanted hash given the INT32 word
    k2 = (np.arange(300, dtype=np.int64) % 7 - 3).astype(np.int32)
    rng = np.random.default_rng(8)
    h2 = (rng.integers(0, 1 << 48, 300, dtype=np.uint64) << U64(16)) | U64(FIRST_CAPACITY - 4) | (np.arange(300, dtype=np.uint64) % U64(4))
    k1 = ht_hash_inverse(h2, 0, later_kws=[k2.astype(np.int64).view(U64)])
    idx = np.arange(n_small) % 300
    add(_pattern("ids_two_keys_wrap_last_group_300", "ids_two_keys", _as_i64(k1[idx]), n_small, ids_stats(300),
                 {"id_group": FIRST_CAPACITY - 4, "distinct": 300}, extra_cols=[Column(I32, k2[idx], None)]))

    # ---- key-range partitions: a STRING key over a 5000-entry dictionary, placed codes ----
    dictionary = [f"s{i:04d}" for i in range(5000)]
    kr_route, gp, nparts = dense_shape(len(dictionary) + 1)
    assert kr_route == "dense_key_range"
    kr = stats(kr_route, 0, gp, nparts)

    def key_range(name, codes, valid=None):
        n = len(codes)
        add(Pattern(name, "key_range", [Column(S, codes.astype(np.int32), valid, dictionary)], values_for(n), [kr] * 3,
                    {"part_groups": gp, "parts": nparts}))

    edges = np.array([c for p in range(nparts - 1) for c in ((p + 1) * gp - 1, (p + 1) * gp)])
    key_range("key_range_partition_edges", _cyclic(edges, n_small))
    key_range("key_range_partial_last_partition", _cyclic(np.arange((nparts - 1) * gp, len(dictionary)), n_small))
    key_range("key_range_one_partition", _cyclic(np.arange(3 * gp, 4 * gp), n_small))
    codes = _cyclic(np.arange(0, 2 * gp, 3), n_small)
    key_range("key_range_null_alone_in_its_partition", codes, valid=np.arange(n_small) % 5 != 2)

    # ---- hash-partitioned: a forced first execution has 64 partitions x 256 buckets; the later ones size from the key count ----
    for route, lines in (("hp_lines", True), ("hp_records", False)):
        tag = "lines" if lines else "records"
        first = stats("hash_partitioned_host", 0, 1 << HP_FIRST_SHIFT, HP_FIRST_PARTS)

        def later(keys_seen):
            parts, buckets = hp_known_shape(keys_seen)
            return stats("hash_partitioned_host", 0, buckets, parts)

        k160 = keys_with_hp_top_bits(0xA7, 8, 160, 10)
        add(_pattern(f"hp_{tag}_five_eighths_160", route, _as_i64(_cyclic(k160, n_small)), n_small, [first, later(160), later(160)],
                     {"top_bits": (0xA7, 8), "distinct": 160}))
        ids300 = stats("dense_ids", 0, *ids_shape(300))
        k6 = keys_with_hp_top_bits(0x2B, 6, 300, 11, next_bits=np.arange(300) % 4, nnext=2)
        add(_pattern(f"hp_{tag}_overflow_then_256_partitions", route, _as_i64(_cyclic(k6, n_small)), n_small,
                     [dict(ids300, abandoned=2), later(300), later(300)], {"top_bits": (0x2B, 6), "distinct": 300, "next2_spread": True}))
        k10 = keys_with_hp_top_bits(0x155, 10, 300, 12)
        add(_pattern(f"hp_{tag}_overflow_at_every_partition_count", route, _as_i64(_cyclic(k10, n_small)), n_small,
                     [dict(ids300, abandoned=2), dict(ids300, abandoned=1), ids300], {"top_bits": (0x155, 10), "distinct": 300}))
        # the last bucket: the records layout takes the hash bits below the partition bits (6 and, later, 8 of them: bits 7 .. 16
        # all ones serve both), the lines layout the 32-bit fold
        if lines:
            kw = keys_with_hp_top_bits(0x3C, 8, 100, 13, line_bucket=255)
            claim = {"top_bits": (0x3C, 8), "line_bucket": 255, "distinct": 100}
        else:
            kw = keys_with_hp_top_bits((0x0F << 10) | 0x3FF, 16, 100, 13)
            claim = {"top_bits": ((0x0F << 10) | 0x3FF, 16), "record_bucket": 255, "distinct": 100}
        add(_pattern(f"hp_{tag}_wrap_last_bucket_100", route, _as_i64(_cyclic(kw, n_small)), n_small, [first, later(100), later(100)], claim))
        # two scatter tiles and a ragged tail: per tile, the records of a partition number 0, 1, R - 1, R, R + 1, ..
        R = hp_line_records(1)
        n_t = 2 * SCATTER_TILE_ROWS + 17
        runs0 = {0: R + 1, 2: R, 3: 1, 4: R - 1, 6: 2 * R, 7: 2 * R + 1}             # partition 1 and 5: empty between full ones
        runs1 = {0: R - 1, 1: R, 4: 1, 6: R + 1}                                     # 0 and 4 go on from a partial line (the carry)
        part = np.full(n_t, 63, np.int64)                                            # the rest: one long run in the last partition
        for t, runs in enumerate((runs0, runs1)):
            pos = t * SCATTER_TILE_ROWS + 5
            for p_, cnt in runs.items():                                             # interleaved with the filler, not adjacent
                part[pos:pos + 3 * cnt:3] = p_
                pos += 3 * cnt + 1
        part[2 * SCATTER_TILE_ROWS:] = np.arange(17) % 3 + 8                          # the tail: partitions 8, 9, 10
        # top 8 bits p << 2: partition p of 64 on the first execution, 4 p of 256 later -- the empty partitions stay between the full ones
        per_part = {int(p_): keys_with_hp_top_bits(int(p_) << 2, 8, 3, 100 + int(p_)) for p_ in np.unique(part)}
        seen = {int(p_): 0 for p_ in np.unique(part)}
        keys_t = np.zeros(n_t, U64)
        for i, p_ in enumerate(part.tolist()):                                       # the 1st, 2nd, 3rd, 1st .. key of its partition
            keys_t[i] = per_part[p_][seen[p_] % 3]
            seen[p_] += 1
        ndist = len(np.unique(keys_t))
        add(_pattern(f"hp_{tag}_tile_runs", route, _as_i64(keys_t), n_t, [first, later(ndist), later(ndist)],
                     {"tile_runs": (runs0, runs1), "row_partition": part, "R": R, "distinct": ndist}))

    # ---- device finish: the groups are ordered by first row with a radix sort over as many 4-bit digits as nrows has ----
    dev_first = stats("hash_partitioned_device", 0, 1 << HP_FIRST_SHIFT, HP_FIRST_PARTS)
    for n in (4096, 4097, 65536, 65537):
        g = 64
        keys = np.zeros(n, np.int64)
        keys[:g - 1] = 5000 - 3 * np.arange(g - 1)                 # first rows 0 .. 62 in descending key order
        keys[g - 1:] = keys[np.arange(g - 1, n) % (g - 1)]
        keys[n - 1] = 5000 - 3 * (g - 1)                           # the smallest key: its first (and only) row is the batch's last
        parts, buckets = hp_known_shape(g)
        dev_later = stats("hash_partitioned_device", 0, buckets, parts)
        add(_pattern(f"hp_device_finish_{n}", "hp_device", keys, n, [dev_first, dev_later, dev_later], {"distinct": g, "last_row_group": True}))
    return pats


_PATTERNS: Optional[Dict[str, Pattern]] = None


def patterns() -> Dict[str, Pattern]:
    """Every pattern, built once per process and shared (nobody changes them)."""
    global _PATTERNS
    if _PATTERNS is None:
        _PATTERNS = build_patterns()
    return _PATTERNS


PATTERN_NAMES = [
    "lds_window_full_32", "lds_window_overflow_33", "lds_window_overflow_33_spills_to_global", "lds_wrap_last_slot_20",
    "lds_null_and_zero_share_the_key_word",
    "global_wrap_300", "global_probe_limit_4097", "global_half_full_32767", "global_half_full_32768",
    "ids_wrap_last_line_300", "ids_first_table_32767", "ids_first_table_32768", "ids_domain_4096", "ids_domain_4097",
    "ids_two_keys_wrap_last_group_300",
    "key_range_partition_edges", "key_range_partial_last_partition", "key_range_one_partition", "key_range_null_alone_in_its_partition",
] + [f"hp_{tag}_{c}" for tag in ("lines", "records") for c in (
    "five_eighths_160", "overflow_then_256_partitions", "overflow_at_every_partition_count", "wrap_last_bucket_100", "tile_runs")
] + [f"hp_device_finish_{n}" for n in (4096, 4097, 65536, 65537)]
