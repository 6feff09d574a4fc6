"""A vectorised reference for the window operator: the rows and values of ``WindowOperator``'s host branch as columns, in
numpy -- for inputs of millions of rows, which the host branch (boxed rows in Python lists) cannot serve.

Pure numpy: no oracle, no GPU.  tests/test_window_cpu.py proves it equal to the host branch value for value; the device
tests rely on that proof.

The sort is ``np.lexsort`` (stable) on comparator-equivalent images: per key the dense rank of (validity, value) in
``compareValues`` order (NULL = rank 0; DOUBLE in ``Double.compareTo`` order with every NaN one value and -0.0 below 0.0;
STRING by UTF-16 code units), negated for a descending key, which also puts NULL last.  Boundary flags compare those ranks
between neighbours, ``np.maximum.accumulate`` gives every row the index of its partition's first row, and the running
aggregates are per-partition cumulative operations in row order starting from 0.0 (a partition of one row is its own
value, so only partitions of two rows and more are walked one by one).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from queryengine_amd import Column, DataType
from queryengine_amd import native as N

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
T, TRIP = N.WIN_TILE_ROWS, N.WIN_TRIP_TILES
RANKS = (N.WIN_ROW_NUMBER, N.WIN_RANK, N.WIN_DENSE_RANK)
NUMERIC = (N.WIN_SUM, N.WIN_MIN, N.WIN_MAX, N.WIN_AVG)
SHIFTS = (N.WIN_LAG, N.WIN_LEAD)


@dataclass
class Expected:
    """One expected output column: validity is always an array; `nullable` says whether the device column carries one."""
    type: DataType
    data: np.ndarray
    valid: np.ndarray
    nullable: bool
    dictionary: Optional[List[str]] = None
    zero_at: Optional[np.ndarray] = None      # rows whose value must be zero: a LAG / LEAD beyond the partition's edge, an
                                              # aggregate before the partition's first valid value


def _valid(c: Column) -> np.ndarray:
    return c.valid if c.valid is not None else np.ones(len(c), dtype=bool)


def total_order(x: np.ndarray) -> np.ndarray:
    """int64 whose order is Double.compareTo's: -0.0 below 0.0, every NaN one value above +inf."""
    bits = np.ascontiguousarray(x, dtype=np.float64).view(np.int64).copy()
    bits[np.isnan(x)] = 0x7ff8000000000000
    return bits ^ ((bits >> 63) & 0x7fffffffffffffff)


def key_rank(c: Column) -> np.ndarray:
    """Dense rank of every row's key value in compareValues order, NULL = 0."""
    valid = _valid(c)
    if c.type == D:
        image = total_order(c.data)
    elif c.type == S:
        order = sorted(set(c.dictionary), key=lambda s: s.encode("utf-16-be", "surrogatepass"))
        rank = {s: i for i, s in enumerate(order)}
        table = np.array([rank[s] for s in c.dictionary] + [0], dtype=np.int64)
        image = table[np.where(valid, c.data, len(c.dictionary))]
    else:
        image = c.data.astype(np.int64)
    out = np.zeros(len(c), dtype=np.int64)
    if valid.any():
        _, inv = np.unique(image[valid], return_inverse=True)
        out[valid] = inv.reshape(-1) + 1
    return out


def _to_double(c: Column) -> np.ndarray:
    return c.data.astype(np.float64)


def _running(v: np.ndarray, valid: np.ndarray, start: np.ndarray, pstart: np.ndarray, fn: int) -> Tuple[np.ndarray, np.ndarray]:
    """(values, count of valid values so far) of one running aggregate; values are meaningless where the count is 0."""
    n = len(v)
    cs = np.cumsum(valid.astype(np.int64))
    count = cs - (cs[start] - valid[start]) if n else cs
    out = np.where(valid, v, 0.0) + 0.0 if fn in (N.WIN_SUM, N.WIN_AVG) else np.where(valid, v, 0.0)   # partitions of one row
    begins = np.nonzero(pstart)[0]
    ends = np.append(begins[1:], n)
    for b, e in zip(begins[ends - begins > 1], ends[ends - begins > 1]):
        x, ok = v[b:e], valid[b:e]
        if fn in (N.WIN_SUM, N.WIN_AVG):
            with np.errstate(invalid="ignore"):                                           # inf + -inf
                out[b:e] = np.cumsum(np.concatenate([[0.0], np.where(ok, x, 0.0)]))[1:]  # in row order from 0.0
        else:
            keys = total_order(x)
            nan = np.logical_or.accumulate(ok & np.isnan(x))                              # NaN wins
            if fn == N.WIN_MIN:
                run = np.minimum.accumulate(np.where(ok, keys, np.iinfo(np.int64).max))
            else:
                run = np.maximum.accumulate(np.where(ok, keys, np.iinfo(np.int64).min))
            seen = np.logical_or.accumulate(ok)
            run = np.where(seen & ~nan, run, 0)
            vals = (run ^ ((run >> 63) & 0x7fffffffffffffff)).view(np.float64).copy()
            vals[nan] = np.nan
            out[b:e] = vals
    if fn == N.WIN_AVG:
        out = out / np.maximum(count, 1)
    return out, count


def window_reference(cols: Sequence[Column], nullable: Sequence[bool], partition_by: Sequence[int], order_by: Sequence,
                     functions: Sequence) -> Tuple[List[Expected], np.ndarray, int]:
    """(expected output columns, perm, partitions): perm[j] = input row that stands at output row j.  `nullable[c]` = the
    input column carries a validity bitmap (``Column`` drops one that is all ones)."""
    n = len(cols[0])
    keys = [(int(c), False) for c in partition_by] + [(int(c), bool(d)) for c, d in order_by]
    ranks = [key_rank(cols[c]) for c, _ in keys]
    if keys:
        perm = np.lexsort([(-r if d else r) for r, (_, d) in zip(ranks, keys)][::-1]).astype(np.int64)
    else:
        perm = np.arange(n, dtype=np.int64)
    j = np.arange(n, dtype=np.int64)
    pstart, peer = j == 0, j == 0
    for k, r in enumerate(ranks):
        s = r[perm]
        diff = np.concatenate([[False], s[1:] != s[:-1]]) if n else np.zeros(0, dtype=bool)
        if k < len(partition_by):
            pstart = pstart | diff
        peer = peer | diff
    peer = peer | pstart
    start = np.maximum.accumulate(np.where(pstart, j, 0)) if n else j
    first_peer = np.maximum.accumulate(np.where(peer, j, 0)) if n else j
    out: List[Expected] = []
    sorted_cols = []
    for c, nl in zip(cols, nullable):
        sc = Column(c.type, c.data[perm], _valid(c)[perm], c.dictionary)
        sorted_cols.append(sc)
        out.append(Expected(c.type, sc.data, _valid(sc), bool(nl), c.dictionary))
    ones = np.ones(n, dtype=bool)
    for f in functions:
        fn, col, offset = (tuple(f) + (0, 0))[:3]
        if fn == N.WIN_ROW_NUMBER:
            out.append(Expected(I64, j - start + 1, ones, False))
        elif fn == N.WIN_RANK:
            out.append(Expected(I64, first_peer - start + 1, ones, False))
        elif fn == N.WIN_DENSE_RANK:
            cp = np.cumsum(peer.astype(np.int64))
            out.append(Expected(I64, (cp - cp[start] + 1) if n else cp, ones, False))
        elif fn in SHIFTS:
            src = sorted_cols[col]
            t = j - offset if fn == N.WIN_LAG else j + offset
            ok = (t >= 0) & (t < n)
            tt = np.where(ok, t, 0)
            if n:
                ok = ok & (start[tt] == start)
                data = np.where(ok, src.data[tt], np.zeros(1, dtype=src.data.dtype))
                valid = ok & _valid(src)[tt]
            else:
                data, valid = src.data, ok
            out.append(Expected(src.type, data, valid, True, src.dictionary, ~ok))
        elif fn == N.WIN_COUNT:
            valid = _valid(sorted_cols[col])
            cs = np.cumsum(valid.astype(np.int64))
            out.append(Expected(D, ((cs - (cs[start] - valid[start])) if n else cs).astype(np.float64), ones, False))
        else:
            src = sorted_cols[col]
            if src.type not in (D, I64, I32):
                raise ValueError("SUM / MIN / MAX / AVG need a numeric column")
            vals, count = _running(_to_double(src), _valid(src), start, pstart, fn)
            out.append(Expected(D, np.where(count > 0, vals, 0.0), count > 0, True, None, count == 0))
    return out, perm, int(pstart.sum())


def assert_window_output(result, want: Sequence[Expected], what: str = "") -> None:
    """Every column of a device result against the expectation, in full: type, nullability, dictionary, validity, and the
    values where valid -- by bits, except that any NaN equals any NaN; where `zero_at` says so the value must be zero."""
    assert result.ncols == len(want), f"{what}: {result.ncols} columns, want {len(want)}"
    for k, w in enumerate(want):
        name = f"{what}: column {k} ({w.type.name})"
        view = result.view(k)
        g = result.column_to_host(k)
        assert g.type == w.type, f"{name}: type {g.type.name}"
        assert bool(view.nullable) == w.nullable, f"{name}: nullable {bool(view.nullable)}, want {w.nullable}"
        assert g.dictionary == w.dictionary, f"{name}: dictionary differs"
        assert len(g) == len(w.data), f"{name}: {len(g)} rows, want {len(w.data)}"
        gv = g.valid if g.valid is not None else np.ones(len(g), dtype=bool)
        bad = np.nonzero(gv != w.valid)[0]
        assert bad.size == 0, f"{name}: validity differs at {bad.size} rows, first {bad[:8]} (got {gv[bad[:8]]})"
        if w.type == D:
            gd, wd = g.data.view(np.uint64), np.ascontiguousarray(w.data, dtype=np.float64).view(np.uint64)
            differ = (gd != wd) & ~(np.isnan(g.data) & np.isnan(w.data))
        else:
            gd, wd = g.data, w.data
            differ = gd != wd
        bad = np.nonzero(differ & w.valid)[0]
        assert bad.size == 0, f"{name}: values differ at {bad.size} rows, first {bad[:8]}: got {g.data[bad[:8]]!r} want {w.data[bad[:8]]!r}"
        if w.zero_at is not None:
            bad = np.nonzero(w.zero_at & (gd != 0))[0]
            assert bad.size == 0, f"{name}: no zeroed value under NULL at {bad.size} rows, first {bad[:8]}: {g.data[bad[:8]]!r}"
