"""Placed key images for the shared radix sort and the top-k select, and a plain numpy reference of what they must return.

The sort decides by the BITS of its key images: a 4-bit pass is skipped when its nibble is the same in
every image, a radix block is 1024 rows in 4 rounds of 256 with one ballot per wave, the select walks 256 bins to the one
that holds rank k and stops at `below + bucket <= max(1.25 k, min(16 384, n/16))`.  Random key pools leave those places to
chance, so the patterns here PLACE the images: an INT64 key whose value is `image ^ 2^63` gives control of all 64 bits.

Everything is written from the documented order and the documented steps, not from the kernels.  Nothing here touches the
GPU, the native library or the C oracle.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from queryengine_amd import Column, DataType

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
U = np.uint64
TOP = U(1 << 63)
ONES = U(0xFFFFFFFFFFFFFFFF)
CANONICAL_NAN = U(0x7FF8000000000000)         # what Double.doubleToLongBits gives for every NaN
BLOCK, ROUND, WAVE = 1024, 256, 64             # rows of a radix block, of one of its four rounds, of a wave
STOP_FLOOR = 16384


# ---- the order -----------------------------------------------------------------------------------------------------------

def utf16_ranks(dictionary: Sequence[str]) -> np.ndarray:
    """Dense rank (from 0) of every dictionary entry in String.compareTo order: UTF-16 code units, a prefix first.  The
    big-endian bytes of the code units compare like the units do."""
    units = [s.encode("utf-16-be", "surrogatepass") for s in dictionary]
    rank = {u: r for r, u in enumerate(sorted(set(units)))}
    return np.array([rank[u] for u in units], dtype=np.uint64)


def image(column: Column, descending: bool) -> Tuple[np.ndarray, np.ndarray]:
    """(u64 image, validity) of a key column in one direction: unsigned order of the images = order of the values.
    DOUBLE: below zero the greater magnitude is the smaller value, -0.0 sits right under 0.0, every NaN is the one value
    above +inf.  INT64 / INT32: the distance from the smallest INT64.  STRING: the UTF-16 rank of the entry.  BOOLEAN:
    false 0, true 1.  NULL: image 0; the validity says on which side of the values it goes.  Descending: the complement."""
    n = len(column)
    valid = np.ones(n, dtype=bool) if column.valid is None else column.valid.astype(bool)
    t = column.type
    if t == D:
        bits = np.ascontiguousarray(column.data, dtype=np.float64).view(np.uint64)
        magnitude = bits & (TOP - U(1))
        negative = (bits >> U(63)) == U(1)
        img = np.where(negative, (TOP - U(1)) - magnitude, TOP + magnitude)
        img[magnitude > U(0x7FF0000000000000)] = TOP + CANONICAL_NAN
    elif t in (I64, I32):
        img = column.data.astype(np.int64).view(np.uint64) + TOP          # wraps: value - INT64_MIN
    elif t == S:
        ranks = utf16_ranks(column.dictionary)
        img = ranks[column.data] if len(ranks) else np.zeros(n, dtype=np.uint64)
    else:
        img = column.data.astype(np.uint64)
    img = np.where(valid, img, U(0)).astype(np.uint64)
    return (~img if descending else img), valid


def expected_order(columns: Sequence[Column], keys: Sequence[Tuple[int, bool]], limit: Optional[int] = None) -> np.ndarray:
    """Row ids in ORDER BY order: one stable argsort per key from the last to the first; NULL first ascending, last
    descending; ties in input order."""
    n = len(columns[0])
    order = np.arange(n, dtype=np.int64)
    for c, desc in reversed(list(keys)):
        img, valid = image(columns[c], desc)
        order = order[np.argsort(img[order], kind="stable")]
        null_class = ~valid if desc else valid                        # ascending: NULL (False) first; descending: NULL (True) last
        order = order[np.argsort(null_class[order], kind="stable")]
    return order if limit is None else order[:max(0, limit)]


def varying_nibbles(images: np.ndarray) -> List[int]:
    """The 4-bit digits (0 = least significant) that are not the same in every image."""
    if len(images) == 0:
        return []
    var = int(np.bitwise_or.reduce(images)) & ~int(np.bitwise_and.reduce(images))
    return [d for d in range(16) if (var >> (4 * d)) & 15]


def expected_radix_passes(columns: Sequence[Column], keys: Sequence[Tuple[int, bool]], rows: Optional[np.ndarray] = None) -> int:
    """Passes of the multi-key sort over `rows` (default: all): per key one pass per varying nibble of its images over
    those rows, and one more when the column carries a validity bitmap.  `rows` is an index array, not a row count m: the
    candidates of a top-k selection are scattered over the row range, not a prefix of it."""
    total = 0
    for c, desc in keys:
        img, _ = image(columns[c], desc)
        total += len(varying_nibbles(img if rows is None else img[rows]))
        total += 1 if columns[c].valid is not None else 0
    return total


# ---- the top-k select ------------------------------------------------------------------------------------------------------

@dataclass
class Selection:
    path: str                   # "select" or "sort"
    c: int                      # candidates the selection found (n when it never ran)
    select_passes: int
    candidates: np.ndarray      # row ids, ascending
    bins: List[int] = field(default_factory=list)     # the digit each pass settled on
    stop_cap: int = 0
    stopped: bool = False       # the stop rule ended it (not the lack of further digits)

    @property
    def sorted_rows(self) -> int:
        return len(self.candidates)


def stop_cap(n: int, k: int) -> int:
    """below + bucket <= max(1.25 k, min(16 384, n/16)), on whole rows."""
    return max(k + k // 4, min(STOP_FLOOR, n // 16))


def select_model(images: np.ndarray, n: int, k: int) -> Selection:
    """DESIGN 3.3b step 2 on the host.  `images`: the first key's images of all n rows in the sort's direction (NULL = 0
    ascending, all ones descending).  k is the number of rows to return (LIMIT already clamped to n)."""
    everything = np.arange(n, dtype=np.int64)
    if not (0 < k < n and k <= n // 2):
        return Selection("sort", n, 0, everything)
    var = int(np.bitwise_or.reduce(images)) & ~int(np.bitwise_and.reduce(images))
    cap = stop_cap(n, k)
    inside = np.ones(n, dtype=bool)          # rows whose digits so far equal the ones settled on
    lower = np.zeros(n, dtype=bool)          # rows that fell below them
    rank, below, passes, bins, stopped = k, 0, 0, [], False
    for byte in range(7, -1, -1):
        if (var >> (8 * byte)) & 255 == 0:
            continue
        digit = ((images >> U(8 * byte)) & U(255)).astype(np.int64)
        counts = np.bincount(digit[inside], minlength=256)
        through = np.cumsum(counts)
        b = int(np.searchsorted(through, rank, side="left"))          # the first bin whose running count reaches the rank
        before = int(through[b] - counts[b])
        lower |= inside & (digit < b)
        inside &= digit == b
        below += before
        rank -= before
        passes += 1
        bins.append(b)
        if below + int(counts[b]) <= cap:
            stopped = True
            break
    cand = np.nonzero(lower | inside)[0].astype(np.int64)
    c = len(cand)
    if c <= n // 2:
        return Selection("select", c, passes, cand, bins, cap, stopped)
    return Selection("sort", c, passes, everything, bins, cap, stopped)


def expected_stats(columns: Sequence[Column], keys: Sequence[Tuple[int, bool]], limit: Optional[int] = None) -> Dict[str, object]:
    """What last_sort_stats() must report for this call."""
    n = len(columns[0])
    nout = n if limit is None or limit > n else limit
    if nout <= 0:
        return {"path": "sort", "sorted_rows": 0, "radix_passes": 0, "select_passes": 0}
    sel = select_model(image(columns[keys[0][0]], keys[0][1])[0], n, nout)
    return {"path": sel.path, "sorted_rows": sel.sorted_rows, "radix_passes": expected_radix_passes(columns, keys, sel.candidates),
            "select_passes": sel.select_passes}


# ---- columns from images ---------------------------------------------------------------------------------------------------

def with_validity(column: Column, valid: np.ndarray) -> Column:
    """A copy of `column` with exactly this validity bitmap -- also an all-true one, which Column() itself would drop.
    The argument is left as it is."""
    out = Column(column.type, column.data, None, column.dictionary)
    out.valid = np.ascontiguousarray(valid, dtype=np.bool_)
    return out


def int64_key(images: np.ndarray, valid: Optional[np.ndarray] = None, descending: bool = False) -> Column:
    """The INT64 column whose image in the given direction is `images`."""
    asc = ~images if descending else images
    col = Column(I64, (asc.astype(np.uint64) ^ TOP).view(np.int64))
    return col if valid is None else with_validity(col, valid)


def double_key(bits: np.ndarray, valid: Optional[np.ndarray] = None) -> Column:
    col = Column(D, np.ascontiguousarray(bits, dtype=np.uint64).view(np.float64))
    return col if valid is None else with_validity(col, valid)


# ---- patterns: all return u64 images ---------------------------------------------------------------------------------------

BASE = 0xA5C396E17B2D4F08          # a constant with both bit values in most nibbles: what a skipped pass must leave alone


def place(digits: np.ndarray, d: int, base: int = 0) -> np.ndarray:
    """Images that hold digits[i] in nibble d and the bits of `base` everywhere else."""
    rest = U(base & ~(15 << (4 * d)) & 0xFFFFFFFFFFFFFFFF)
    return (digits.astype(np.uint64) << U(4 * d)) | rest


def _all_values(rng, n: int, count: int) -> np.ndarray:
    """n random draws from range(count) that hold every value at least once."""
    v = rng.integers(0, count, n)
    v[rng.permutation(n)[:count]] = np.arange(count)
    return v


def one_nibble(n: int, d: int, rng, base: int = 0) -> np.ndarray:
    return place(_all_values(rng, n, 16), d, base)


def one_bit(n: int, b: int, rng, base: int = 0) -> np.ndarray:
    rest = U(base & ~(1 << b) & 0xFFFFFFFFFFFFFFFF)
    return (_all_values(rng, n, 2).astype(np.uint64) << U(b)) | rest


def two_nibbles(n: int, a: int, b: int, rng, base: int = 0) -> np.ndarray:
    rest = U(base & ~(15 << (4 * a)) & ~(15 << (4 * b)) & 0xFFFFFFFFFFFFFFFF)
    return (_all_values(rng, n, 16).astype(np.uint64) << U(4 * a)) | (_all_values(rng, n, 16).astype(np.uint64) << U(4 * b)) | rest


def _stray(n: int, last: bool) -> np.ndarray:
    i = np.arange(n)
    at = (i % BLOCK == BLOCK - 1) | (i == n - 1) if last else (i % BLOCK == 0)
    return np.where(at, 1 + (i // BLOCK) % 15, 0)


LAYOUTS: Dict[str, Callable[[int], np.ndarray]] = {
    "block_constant": lambda n: (np.arange(n) // BLOCK) % 16,
    "round_cyclic": lambda n: (np.arange(n) // ROUND) % 16,
    "wave_cyclic": lambda n: (np.arange(n) // WAVE) % 16,
    "lane_cyclic": lambda n: np.arange(n) % 16,
    "sorted": lambda n: np.arange(n) * 16 // max(n, 1),
    "reversed": lambda n: 15 - np.arange(n) * 16 // max(n, 1),
    "one_stray_row_last": lambda n: _stray(n, True),
    "one_stray_row_first": lambda n: _stray(n, False),
}


def layout(name: str, n: int, d: int = 0, base: int = 0) -> np.ndarray:
    """The digit layout `name` in nibble d."""
    return place(LAYOUTS[name](n), d, base)


def select_buckets(n: int, sizes: Sequence[int], rng, second: Optional[Tuple[int, int]] = None) -> np.ndarray:
    """Images whose top byte is b in exactly sizes[b] rows, shuffled over the row range; `second` = (bucket, values) gives
    the rows of that bucket `values` different second bytes, every other bit stays 0."""
    sizes = np.asarray(sizes, dtype=np.int64)
    assert len(sizes) == 256 and int(sizes.sum()) == n and (sizes >= 0).all()
    top = np.repeat(np.arange(256), sizes)
    rng.shuffle(top)
    img = top.astype(np.uint64) << U(56)
    if second is not None:
        bucket, values = second
        rows = np.nonzero(top == bucket)[0]
        img[rows] |= _all_values(rng, len(rows), values).astype(np.uint64) << U(48)
    return img


def sizes_from(n: int, placed: Dict[int, int], rest_bin: int = 255) -> np.ndarray:
    """256 bucket sizes: the placed ones, and whatever is left of n in `rest_bin`."""
    sizes = np.zeros(256, dtype=np.int64)
    for b, s in placed.items():
        sizes[b] = s
    sizes[rest_bin] += n - int(sizes.sum())
    assert sizes[rest_bin] >= 0
    return sizes


# ---- the top-k cases: one table for the host checks and the device run ---------------------------------------------------------

N_SELECT = 40001
WALK_BUCKETS = (0, 2, 3, 4, 127, 254, 255)


def walk_sizes(n: int = N_SELECT) -> np.ndarray:
    """Bucket sizes for the rank walk: empty buckets next to the targets (1, 5, 126, 128, 253), small ones in between, and
    most of the rows in bucket 255 so that every running count through 254 stays under n/2."""
    placed = {0: 37, 2: 50, 3: 41, 4: 29, 127: 300, 254: 100}
    for j in range(6, 126):
        placed[j] = 3 + (j * 7) % 11
    for j in range(129, 253):
        placed[j] = 2 + (j * 5) % 9
    return sizes_from(n, placed)


# the first bin a correct walk settles on, for k = count through bucket b (+0) and one more (+1); None: no selection runs
WALK_TARGET = {(0, 0): 0, (0, 1): 2, (2, 0): 2, (2, 1): 3, (3, 0): 3, (3, 1): 4, (4, 0): 4, (4, 1): 6, (127, 0): 127, (127, 1): 129,
               (254, 0): 254, (254, 1): 255, (255, 0): None, (255, 1): None}


@dataclass
class SelectCase:
    name: str
    build: Callable[[], Tuple[List[Column], List[Tuple[int, bool]], int]]     # -> (key columns, keys, limit)
    intent: Dict[str, object]                                                # what the case is placed to do


def _walk_case(b: int, plus: int, desc: bool):
    def build():
        rng = np.random.default_rng(1000 + b)
        sizes = walk_sizes()
        img = select_buckets(N_SELECT, sizes, rng)
        return [int64_key(img, descending=desc)], [(0, desc)], int(np.cumsum(sizes)[b]) + plus
    target = WALK_TARGET[(b, plus)]
    intent = {"select_passes": 0, "path": "sort"} if target is None else {"select_passes": 1, "bins": [target], "path": "sort" if target == 255 else "select"}
    return SelectCase(f"walk-b{b}+{plus}-{'desc' if desc else 'asc'}", build, intent)


def _stop_case(name: str, k: int, below: int, bucket: int, intent: Dict[str, object], desc: bool = False):
    def build():
        rng = np.random.default_rng(2000 + bucket)
        sizes = np.full(256, 0, dtype=np.int64)
        sizes[3], sizes[7] = below, bucket
        rest = N_SELECT - below - bucket
        sizes[8:] = rest // 248
        sizes[255] += rest - int(sizes[8:].sum())
        img = select_buckets(N_SELECT, sizes, rng, second=(7, 256))
        return [int64_key(img, descending=desc)], [(0, desc)], k
    return SelectCase(name, build, intent)


def _gate_case(name: str, n: int, k: int, first: int, spread: int, intent: Dict[str, object]):
    """The lowest `spread` buckets hold `first` rows together, the rest lies above them."""
    def build():
        rng = np.random.default_rng(3000 + n + first + spread)
        sizes = np.zeros(256, dtype=np.int64)
        sizes[:spread] = first // spread
        sizes[spread - 1] += first - int(sizes[:spread].sum())
        sizes[spread:] = (n - first) // (256 - spread)
        sizes[255] += n - int(sizes.sum())
        img = select_buckets(n, sizes, rng)
        return [int64_key(img)], [(0, False)], k
    return SelectCase(name, build, intent)


N_FOLD = 128 * 300 + 1          # n = 1 (mod 128): the last pair holds one row, the last wave one lane
FOLD_TARGET = 5


def fold_images(n: int = N_FOLD) -> np.ndarray:
    """First byte by LANE of the select's histogram (a lane reads rows 2p and 2p + 1): a quarter of the rows with one
    value per wave, then three quarters where lanes alternate with period 2, 3 and 4 between the smallest value and 1, 2,
    3 others.  The smallest value holds far more rows than the stop rule lets through, so a second pass runs in which the
    rows still inside are every 2nd, 3rd or 4th lane; their second byte varies."""
    i = np.arange(n)
    lane = i // 2
    seg = np.minimum((i // 128) * 4 // (n // 128), 3)          # whole waves (128 rows) per segment
    per_wave = 10 + (i // 128) % 3
    digit = np.where(seg == 0, per_wave,
                     np.where(seg == 1, np.array([FOLD_TARGET, 20])[lane % 2],
                              np.where(seg == 2, np.array([FOLD_TARGET, 21, 22])[lane % 3], np.array([FOLD_TARGET, 23, 24, 25])[lane % 4])))
    img = digit.astype(np.uint64) << U(56)
    inside = digit == FOLD_TARGET
    img[inside] |= ((np.nonzero(inside)[0] * 37) % 256).astype(np.uint64) << U(48)
    return img


def _fold_case(desc: bool):
    def build():
        return [int64_key(fold_images(), descending=desc)], [(0, desc)], 100
    return SelectCase(f"fold-{'desc' if desc else 'asc'}", build, {"select_passes": 2, "path": "select", "stopped": True})


def _degenerate_cases() -> List[SelectCase]:
    def equal():
        return [int64_key(np.full(N_SELECT, BASE, dtype=np.uint64))], [(0, False)], 10

    def all_null():
        return [int64_key(np.arange(N_SELECT, dtype=np.uint64), valid=np.zeros(N_SELECT, dtype=bool))], [(0, True)], 10

    def smallest_last():
        rng = np.random.default_rng(4000)
        img = rng.integers(1 << 20, 1 << 62, N_SELECT).astype(np.uint64)
        img[-1] = 7
        return [int64_key(img)], [(0, False)], 1
    return [SelectCase("all-equal", equal, {"select_passes": 0, "path": "sort"}),
            SelectCase("all-null", all_null, {"select_passes": 0, "path": "sort"}),
            SelectCase("k1-smallest-in-the-last-row", smallest_last, {"path": "select"})]


def select_cases() -> List[SelectCase]:
    half_odd, half_even = N_SELECT // 2, (N_SELECT - 1) // 2
    cases = [_walk_case(b, plus, desc) for b in WALK_BUCKETS for plus in (0, 1) for desc in (False, True)]
    cases += [
        # k = 100 at n = 40 001: the cap is min(16 384, n/16) = 2500
        _stop_case("stop-floor-at-cap", 100, 40, 2460, {"select_passes": 1, "stopped": True, "c": 2500, "stop_cap": 2500, "path": "select"}),
        _stop_case("stop-floor-past-cap", 100, 40, 2461, {"select_passes": 2, "stopped": True, "stop_cap": 2500, "path": "select"}),
        _stop_case("stop-floor-at-cap-desc", 100, 0, 2500, {"select_passes": 1, "stopped": True, "c": 2500, "path": "select"}, desc=True),
        # k = 4002: 1.25 k = 5002.5 is the larger term, whole rows: 5002
        _stop_case("stop-k-at-cap", 4002, 3000, 2002, {"select_passes": 1, "stopped": True, "c": 5002, "stop_cap": 5002, "path": "select"}),
        _stop_case("stop-k-past-cap", 4002, 3000, 2003, {"select_passes": 2, "stopped": True, "stop_cap": 5002, "path": "select"}),
    ]
    for n, half in ((N_SELECT, half_odd), (N_SELECT - 1, half_even)):
        cases += [
            _gate_case(f"gate-k-half-n{n}", n, half, half, 100, {"select_passes": 1, "c": half, "path": "select"}),
            _gate_case(f"gate-k-half+1-n{n}", n, half + 1, half, 100, {"select_passes": 0, "path": "sort"}),
            _gate_case(f"gate-c-half-n{n}", n, 100, half, 1, {"select_passes": 1, "c": half, "path": "select"}),
            _gate_case(f"gate-c-half+1-n{n}", n, 100, half + 1, 1, {"select_passes": 1, "c": half + 1, "path": "sort"}),
        ]
    cases += [_fold_case(False), _fold_case(True)]
    return cases + _degenerate_cases()


SELECT_CASES: Dict[str, SelectCase] = {c.name: c for c in select_cases()}
