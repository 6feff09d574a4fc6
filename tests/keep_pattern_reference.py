"""Keep patterns for the fused filter+project kernels, and a plain numpy reference of what they must return.

The fused scan (DESIGN.md 3.1 ring, 3.1b dense, 3.1c local, two-pass) changes behaviour at exact per-chunk kept counts: the
ring spills 64 rows once `run - flushed >= ring - 128` after a 128-row load group, the local form overflows past `fl_ring`
rows per chunk, the look-back has a 64-chunk block level.  Which rows a filter keeps is deterministic in the data, so the
patterns here PLACE the kept rows: a chunk that keeps exactly ring-128 rows, full chunks next to empty ones, only odd rows.

Nothing here touches the GPU or the C oracle: masks, columns and the expected output are numpy only.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from queryengine_amd import Column, DataType

from helpers import Fn, col, fn, num

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING

# qe_options.tuning[5]: the switches that pin one form of the fused executor (qe_internal.h, DebugBit)
RING_BITS = 1024 | 32768 | 524288      # never two-pass, never dense, never local
DENSE_BITS = 16384
TWO_PASS_BITS = 512
LOCAL_BITS = 262144 | 32768 | 1024    # local, and never dense / two-pass: a plan that has kept >= 12 % would move to the dense form


@dataclass(frozen=True)
class Geometry:
    """One geometry of the fused kernel as qe_options.tuning pins it (geometry_of in qe_api.cpp).  `explicit` False: the
    defaults (tuning[0..4] all 0)."""
    name: str
    threads: int
    unroll: int
    subs_per_chunk: int
    ring: int
    explicit: bool = True

    @property
    def sub_rows(self) -> int:
        return 128 * self.unroll

    @property
    def chunk_rows(self) -> int:
        return self.sub_rows * self.subs_per_chunk

    @property
    def tile_rows(self) -> int:
        """Rows of a dense-form tile (one sub-tile per wave of the workgroup) before the LDS budget shrinks it."""
        return self.sub_rows * self.threads // 64

    def dense_tile_rows(self, row_bytes: int) -> int:
        """The dense tile after dense_lds_tile (qe_api.cpp): a parked tile stays within 64 KiB; knobs that tuning pins
        explicitly are left alone."""
        threads, unroll = self.threads, self.unroll
        if not self.explicit:
            while threads // 64 * 128 * unroll * row_bytes > 64 * 1024 and unroll > 1:
                unroll //= 2
            while threads // 64 * 128 * unroll * row_bytes > 64 * 1024 and threads > 128:
                threads //= 2
        return threads // 64 * 128 * unroll

    def tuning(self, bits: int = 0, lookback_k: int = 0, nbuf: int = 0, stores: int = 0, subs: Optional[int] = None) -> List[int]:
        """[threads, unroll, stores, 0, subs + 10000 * (ring / 256), bits, lookback_k, 100 * nbuf]; a 256-entry ring is the default (0)"""
        if self.explicit:
            t = [self.threads, self.unroll, stores, 0, (self.subs_per_chunk if subs is None else subs) + (10000 * (self.ring // 256) if self.ring != 256 else 0)]
        else:
            t = [0, 0, stores, 0, 0 if subs is None else subs]
        return t + [bits, lookback_k, 100 * nbuf]


GEOMETRIES = {g.name: g for g in (
    Geometry("default", 256, 8, 16, 256, explicit=False),
    Geometry("wide", 256, 16, 4, 512),
    Geometry("mid", 128, 8, 8, 512),
    Geometry("small", 256, 2, 4, 256),
    Geometry("small512", 256, 2, 4, 512),
)}


def seam_counts(geo: Geometry) -> List[int]:
    """Kept rows of one chunk around every seam of the spill rule, and around a whole chunk."""
    r, c = geo.ring, geo.chunk_rows
    return [r - 129, r - 128, r - 127, r - 65, r - 64, r - 63, r - 1, r, r + 1, c - 1, c]


def row_counts(geo: Geometry) -> List[int]:
    """One chunk past a level-0 block, a ragged last block of 1 and of 2 chunks, two full blocks plus a tail."""
    c, t = geo.chunk_rows, geo.sub_rows
    return [2 * c + 1, 5 * c + 129, 64 * c, 64 * c + 1, 65 * c + t - 1, 130 * c + 7]


def pattern_id(pattern: Tuple) -> str:
    return "-".join(str(x) for x in pattern)


def _runs(n: int, seed: int, mean_keep: int, mean_drop: int) -> np.ndarray:
    """Alternating geometric runs of kept and dropped rows (clustered random), a dropped run first."""
    rng = np.random.default_rng(seed)
    pairs = int(2.5 * n / (mean_keep + mean_drop)) + 64
    while True:
        lens = np.empty(2 * pairs, dtype=np.int64)
        lens[0::2] = rng.geometric(1.0 / mean_drop, pairs)
        lens[1::2] = rng.geometric(1.0 / mean_keep, pairs)
        if int(lens.sum()) >= n:
            break
        pairs *= 2
    flags = np.zeros(2 * pairs, dtype=bool)
    flags[1::2] = True
    return np.repeat(flags, lens)[:n]


def keep_mask(pattern: Tuple, n: int, geo: Geometry, unit: Optional[int] = None) -> np.ndarray:
    """The rows `pattern` keeps out of n, as a bool array.  `unit`: the rows of a "chunk" where that is not the ring form's
    chunk (a dense tile, a chunk of the local form); default geo.chunk_rows."""
    name, args = pattern[0], pattern[1:]
    c = geo.chunk_rows if unit is None else int(unit)
    idx = np.arange(n, dtype=np.int64)
    mask = np.zeros(n, dtype=bool)
    if name == "all":
        mask[:] = True
    elif name == "none":
        pass
    elif name == "first_row":
        mask[:1] = True
    elif name == "last_row":
        mask[n - 1:] = True
    elif name == "seam_head":          # chunk 1 (chunk 0 knows its prefix) keeps its first k rows
        (k,) = args
        assert 0 <= k <= c and n >= 2 * c
        mask[c:c + k] = True
    elif name == "seam_tail":          # .. its last k rows: the threshold is crossed in the chunk's last groups
        (k,) = args
        assert 0 <= k <= c and n >= 2 * c
        mask[2 * c - k:2 * c] = True
    elif name in ("full_then_empty", "full_then_one"):
        (p,) = args
        mask = (idx // c) % p == 1           # chunks 1, 1 + p, ..: chunk 0 (which knows its prefix) is never the full one
        if name == "full_then_one":    # the other chunks keep exactly their last row (a ragged last chunk: row n - 1)
            mask = mask | (idx % c == c - 1)
            mask[n - 1:] = True
    elif name == "straddle":
        start, length = args
        mask[start:start + length] = True
    elif name == "odd_rows":
        mask = idx % 2 == 1
    elif name == "even_rows":
        mask = idx % 2 == 0
    elif name == "lane63":             # a lane holds rows 2l, 2l + 1 of a 128-row load group
        mask = idx % 128 >= 126
    elif name == "one_per_group":
        mask = idx % 128 == (idx // 128) % 128
    elif name == "one_per_chunk_last":
        mask = idx % c == c - 1
    elif name == "runs":
        seed, mean_keep, mean_drop = args
        mask = _runs(n, seed, mean_keep, mean_drop)
    elif name == "iid":
        seed, p = args
        mask = np.random.default_rng(seed).random(n) < p
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(mask, dtype=bool)


def chunk_counts(mask: np.ndarray, chunk_rows: int) -> np.ndarray:
    """Kept rows per chunk of chunk_rows rows (the last one may be ragged)."""
    n = len(mask)
    nchunks = max(1, -(-n // chunk_rows))
    padded = np.zeros(nchunks * chunk_rows, dtype=np.int64)
    padded[:n] = mask
    return padded.reshape(nchunks, chunk_rows).sum(axis=1)


def spill_model(mask: np.ndarray, geo: Geometry, slack: int = 128) -> Tuple[np.ndarray, np.ndarray]:
    """The ring form's spill rule on the host: a chunk is walked in load groups of 128 rows; a group's kept rows are written
    to the ring, then, while `run - flushed >= ring - slack`, 64 rows leave for the staging slot.  Returns every chunk's
    `flushed`, and the most rows its ring ever had to hold (right after a group's rows were written): more than `ring` would
    overwrite rows that have not been spilled yet.  A model of the rule that qualifies patterns (does this chunk spill?),
    never the expected output of a query."""
    c, r = geo.chunk_rows, geo.ring
    n = len(mask)
    nchunks = max(1, -(-n // c))
    padded = np.zeros(nchunks * c, dtype=np.int64)
    padded[:n] = mask
    groups = padded.reshape(nchunks, c // 128, 128).sum(axis=2)
    run = np.zeros(nchunks, dtype=np.int64)
    flushed = np.zeros(nchunks, dtype=np.int64)
    high = np.zeros(nchunks, dtype=np.int64)
    for g in range(c // 128):
        run += groups[:, g]
        high = np.maximum(high, run - flushed)
        while True:
            over = run - flushed >= r - slack
            if not over.any():
                break
            flushed[over] += 64
    return flushed, high


def spilled_rows(mask: np.ndarray, geo: Geometry) -> np.ndarray:
    """Rows every chunk spills to its staging slot under the shipped rule (spill_model)."""
    return spill_model(mask, geo)[0]


# ---- row shapes ---------------------------------------------------------------------------------------------------------
SHAPES = ("one", "pair", "mixed")
ROW_BYTES = {"one": 8, "pair": 24, "mixed": 4 + 9 + 1 + 4 + 9}   # bytes of a kept row while it waits in LDS / staging
STRINGS = [f"s{i}" for i in range(8)]
_DROP = 1000      # k of a dropped row: 1000 .. 1012, above every literal the filters use


def fl_ring(shape: str, geo: Geometry) -> int:
    """Rows of a chunk slot of the local form: max(ring, 512 for rows of <= 18 bytes, else 256) (qe_codegen.cpp)."""
    return max(geo.ring, 512 if ROW_BYTES[shape] <= 18 else 256)


@dataclass
class Case:
    columns: List[Column]
    filter: object                 # AST of the filter
    projections: list              # ASTs of the projections
    spec: List[Tuple]              # the same projections for expected(): ("col", i) or ("add", i, j)
    mask: np.ndarray               # the rows the filter keeps
    filter_cols: Tuple[int, ...] = (0,)   # the columns the filter compares with its literal


@functools.lru_cache(maxsize=4)
def _noise(n: int):
    """Per-row random bits shared by every case of n rows (the cases differ in k, m and the tagged row ids)."""
    rng = np.random.default_rng(n)
    return rng.random(n), rng.random(n)


def _near(mask: np.ndarray) -> np.ndarray:
    """Dropped rows right next to a kept one (also one load group away)."""
    near = np.zeros(len(mask), dtype=bool)
    for s in (1, 2, 128):
        near[s:] |= mask[:-s]
        near[:-s] |= mask[s:]
    return near & ~mask


def build_case(shape: str, n: int, mask: np.ndarray, tag: int, literal: int = 1) -> Case:
    """Columns, filter and projections of one row shape whose filter keeps exactly `mask`.  `tag` (0 .. 255) goes into bits
    40 .. 47 of every row id: two executions never carry the same values, so a row left in a staging slot or an LDS ring
    by an earlier execution cannot pass for a row of this one."""
    assert len(mask) == n and mask.dtype == bool and 0 <= tag < 256 and 1 <= literal < _DROP
    idx = np.arange(n, dtype=np.int64)
    rid = idx | (np.int64(tag) << np.int64(40))
    u0, u1 = _noise(n)
    drop = _DROP + idx % 13
    K, RID = col("k", 0, I64), col("rid", 1, I64)
    if shape == "one":
        k = np.where(mask, 0, drop)
        return Case([Column(I64, k), Column(I64, rid)], fn(Fn.CMP_LT, K, num(literal)), [RID], [("col", 1)], mask)
    if shape == "pair":
        # k and m are 0 on the kept rows and on two DISJOINT 25 % extras: only the AND keeps exactly `mask`, and the second
        # conjunct and the projections are loaded under a partial exec mask (late materialisation)
        k = np.where(mask | (u0 < 0.25), 0, drop)
        m = np.where(mask | ((u0 >= 0.25) & (u0 < 0.5)), 0, drop)
        d = rid.astype(np.float64) * 0.25
        cols = [Column(I64, k), Column(I64, rid), Column(I64, m), Column(D, d)]
        M, DD = col("m", 2, I64), col("d", 3, D)
        flt = fn(Fn.AND, fn(Fn.CMP_LT, K, num(literal)), fn(Fn.CMP_LT, M, num(literal)))
        return Case(cols, flt, [RID, fn(Fn.ADD, RID, K), DD], [("col", 1), ("add", 1, 0), ("col", 3)], mask, (0, 2))
    if shape == "mixed":
        # k is nullable: NULL (over a 0 that would pass) on dropped rows, most of them right next to kept ones -- about 10 %
        # of the rows that `k < literal` alone would keep; a NULL filter drops the row
        sel = float(mask.mean()) if n else 0.0
        near = _near(mask)
        null = (near & (u0 < 0.35)) | (~mask & (u1 < 0.1 * sel))
        after = np.zeros(n, dtype=bool)
        after[1:] = mask[:-1] & ~mask[1:]
        if after.any():
            null[int(np.argmax(after))] = True     # at least the row that ends the first kept run
        elif not mask.all():
            null[int(np.argmin(mask))] = True      # .. or any dropped row: k is nullable whenever a row is dropped (one plan)
        k = np.where(mask | null, 0, drop)
        a = (idx + 7919 * tag).astype(np.int32)
        d = rid.astype(np.float64) * 0.5
        b = (idx + tag) % 3 == 0
        s = ((idx + tag) % 8).astype(np.int32)
        cols = [Column(I64, k, ~null), Column(I32, a), Column(D, d, u0 >= 0.2), Column(B, b), Column(S, s, None, list(STRINGS)),
                Column(I64, rid, u1 >= 0.15)]
        projs = [col("a", 1, I32), col("d", 2, D), col("b", 3, B), col("s", 4, S), col("v", 5, I64)]
        return Case(cols, fn(Fn.CMP_LT, K, num(literal)), projs, [("col", j) for j in range(1, 6)], mask)
    raise ValueError(shape)


def filter_mask(case: Case, literal: int = 1) -> np.ndarray:
    """The kept rows read back from the COLUMNS (valid AND k < literal, for every filter column): build_case must have made
    them equal to the mask it was given."""
    keep = np.ones(len(case.mask), dtype=bool)
    for j in case.filter_cols:
        c = case.columns[j]
        keep &= c.data < literal
        if c.valid is not None:
            keep &= c.valid
    return keep


def expected(columns: Sequence[Column], mask: np.ndarray, spec: Sequence[Tuple]) -> List[Column]:
    """Projection(Filter(Scan)) in numpy: `col[mask]` for a pass-through projection, integer `+` for ("add", i, j); a row of
    the sum is valid where both operands are."""
    out = []
    for p in spec:
        if p[0] == "col":
            c = columns[p[1]]
            out.append(Column(c.type, c.data[mask], None if c.valid is None else c.valid[mask], c.dictionary))
        elif p[0] == "add":
            x, y = columns[p[1]], columns[p[2]]
            assert x.type == y.type == I64
            valid = None
            if x.valid is not None or y.valid is not None:
                valid = (np.ones(len(mask), bool) if x.valid is None else x.valid) & (np.ones(len(mask), bool) if y.valid is None else y.valid)
            out.append(Column(I64, (x.data + y.data)[mask], None if valid is None else valid[mask]))
        else:
            raise ValueError(p)
    return out
