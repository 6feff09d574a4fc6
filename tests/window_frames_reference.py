"""A numpy restatement of the window operator WITH FRAMES (qe_result_window_frames; ``WindowOperator`` with 5-tuples).

Sorting, partitions, the ranks, LAG / LEAD and the running frame come from tests/window_reference.py.  A framed function is
stated twice:

``slices``  the literal one.  Per row the slice [lo, hi] of the sorted partition is taken: COUNT, MIN and MAX exactly, SUM as
            ``math.fsum`` of the slice's valid values together with sum|x| and c (so the header's bound can be asserted),
            special values by the group-by rules -- a NaN or both infinities in the frame give NaN, one infinity gives that
            infinity, only -0.0 gives +0.0; MIN / MAX let NaN win and order -0.0 below +0.0.
``exact``   for inputs of millions of rows, and only for values that are multiples of 0.5 (plus NaN, the infinities, -0.0):
            every partial sum of such values is exact, so a frame's sum is a difference of exact integer prefix sums -- of the
            REFERENCE's integers; the device may not subtract prefixes -- and MIN / MAX are range queries on a sparse table.
            tests/test_window_frames_cpu.py proves it equal to ``slices``.

Pure numpy: no oracle, no GPU."""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np

from queryengine_amd import DataType
from queryengine_amd import native as N
from queryengine_amd.engine import window_frame_fn

from window_reference import Expected, total_order, window_reference

D = DataType.DOUBLE
UNB = N.FRAME_UNBOUNDED
AGGS = (N.WIN_SUM, N.WIN_COUNT, N.WIN_MIN, N.WIN_MAX, N.WIN_AVG)
VALUES = (N.WIN_FIRST_VALUE, N.WIN_LAST_VALUE)
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def frame_bounds(start: np.ndarray, end: np.ndarray, preceding: int, following: int) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) of every row: the frame clamped to the partition [start, end]."""
    j = np.arange(len(start), dtype=np.int64)
    lo = start if preceding == UNB else np.maximum(start, j - preceding)
    hi = end if following == UNB else np.minimum(end, j + following)
    return lo, hi


def _from_order(keys: np.ndarray) -> np.ndarray:
    return (keys ^ ((keys >> 63) & 0x7fffffffffffffff)).view(np.float64).copy()


def frame_slices(v: np.ndarray, valid: np.ndarray, lo: np.ndarray, hi: np.ndarray, fn: int):
    """(value, count, sum|x|) per row, from the slice [lo, hi] itself.  value: SUM -> fsum (AVG: the same fsum; the caller
    divides), MIN / MAX -> the extreme; meaningless where count == 0."""
    n = len(v)
    out, cnt, absum = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n)
    for j in range(n):
        x = v[lo[j]:hi[j] + 1][valid[lo[j]:hi[j] + 1]]
        cnt[j] = len(x)
        if len(x) == 0 or fn == N.WIN_COUNT:
            continue
        nan = bool(np.isnan(x).any())
        if fn in (N.WIN_SUM, N.WIN_AVG):
            pinf, ninf = bool((x == np.inf).any()), bool((x == -np.inf).any())
            if nan or (pinf and ninf):
                out[j] = np.nan
            elif pinf or ninf:
                out[j] = np.inf if pinf else -np.inf
            else:
                out[j] = math.fsum(x) + 0.0          # only -0.0 -> +0.0
                absum[j] = math.fsum(np.abs(x))
        elif nan:
            out[j] = np.nan                           # NaN wins
        else:
            keys = total_order(x)                     # -0.0 below +0.0
            out[j] = _from_order(np.array([keys.min() if fn == N.WIN_MIN else keys.max()], dtype=np.int64))[0]
    return out, cnt, absum


def _range_count(flags: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    cs = np.concatenate([[0], np.cumsum(flags.astype(np.int64))])
    return cs[hi + 1] - cs[lo]


def _range_extreme(keys: np.ndarray, lo: np.ndarray, hi: np.ndarray, want_max: bool) -> np.ndarray:
    """min / max of keys[lo .. hi] per row through a sparse table (level k holds the extreme of 2^k keys)."""
    op = np.maximum if want_max else np.minimum
    length = hi - lo + 1
    level = np.zeros(len(keys), dtype=np.int64)
    level[length > 0] = np.floor(np.log2(length[length > 0])).astype(np.int64)
    level = np.where((np.int64(1) << level) > length, level - 1, level)      # log2 rounding at exact powers
    out = np.zeros(len(keys), dtype=np.int64)
    table = keys
    for k in range(int(level.max()) + 1 if len(keys) else 0):
        if k > 0:
            half = 1 << (k - 1)
            table = op(table[:-half], table[half:])
        pick = np.nonzero(level == k)[0]
        if pick.size:
            out[pick] = op(table[lo[pick]], table[hi[pick] - (1 << k) + 1])
    return out


def frame_exact(v: np.ndarray, valid: np.ndarray, lo: np.ndarray, hi: np.ndarray, fn: int):
    """As frame_slices, vectorised, for values whose doubles are integers (so every sum is exact)."""
    cnt = _range_count(valid, lo, hi)
    absum = np.zeros(len(v))
    if fn == N.WIN_COUNT:
        return np.zeros(len(v)), cnt, absum
    nan = _range_count(valid & np.isnan(v), lo, hi) > 0
    if fn in (N.WIN_SUM, N.WIN_AVG):
        finite = valid & np.isfinite(v)
        doubled = np.where(finite, v, 0.0) * 2.0
        assert np.array_equal(doubled, np.rint(doubled)) and np.abs(doubled).sum() < 2.0 ** 52, "exact mode needs multiples of 0.5"
        cs = np.concatenate([[0], np.cumsum(doubled.astype(np.int64))])
        ca = np.concatenate([[0], np.cumsum(np.abs(doubled).astype(np.int64))])
        out = (cs[hi + 1] - cs[lo]).astype(np.float64) / 2.0
        absum = (ca[hi + 1] - ca[lo]).astype(np.float64) / 2.0
        pinf, ninf = _range_count(valid & (v == np.inf), lo, hi) > 0, _range_count(valid & (v == -np.inf), lo, hi) > 0
        out = np.where(pinf, np.inf, np.where(ninf, -np.inf, out))
        out = np.where(nan | (pinf & ninf), np.nan, out)
        return out, cnt, np.where(np.isfinite(out), absum, 0.0)
    want_max = fn == N.WIN_MAX
    usable = valid & ~np.isnan(v)
    keys = np.where(usable, total_order(np.where(usable, v, 0.0)), I64_MIN if want_max else I64_MAX)
    run = _range_extreme(keys, lo, hi, want_max)
    some = _range_count(usable, lo, hi) > 0
    out = _from_order(np.where(some, run, 0))
    out[nan] = np.nan
    return out, cnt, absum


def frames_reference(cols, nullable, partition_by, order_by, functions, mode: str = "slices"):
    """(expected output columns, details): details[k] = None, or for a framed SUM / AVG the dict {"sum": fsum of the frame,
    "abs": sum|x|, "count": c} to assert the numeric bound with.  `functions` as ``WindowOperator`` takes them."""
    fns = [window_frame_fn(f) for f in functions]
    n = len(cols[0])
    legacy = [(k, f) for k, f in enumerate(fns) if f[0] not in VALUES and not (f[0] in AGGS and (f[3], f[4]) != (UNB, 0))]
    base, _, _ = window_reference(cols, nullable, partition_by, order_by, [(N.WIN_ROW_NUMBER,)] + [f[:3] for _, f in legacy])
    ncols = len(cols)
    j = np.arange(n, dtype=np.int64)
    start = j - (base[ncols].data.astype(np.int64) - 1)
    begins = np.nonzero(start == j)[0]
    end = (np.append(begins[1:], n) - 1)[np.searchsorted(begins, start)] if n else j
    out: List[Expected] = list(base[:ncols])
    details = []
    from_legacy = {k: base[ncols + 1 + i] for i, (k, _) in enumerate(legacy)}
    ones = np.ones(n, dtype=bool)
    for k, (fn, col, _, preceding, following) in enumerate(fns):
        if k in from_legacy:
            out.append(from_legacy[k])
            details.append(None)
            continue
        lo, hi = frame_bounds(start, end, preceding, following)
        src = base[col]
        if fn in VALUES:
            at = lo if fn == N.WIN_FIRST_VALUE else hi
            out.append(Expected(src.type, src.data[at], src.valid[at], bool(nullable[col]), src.dictionary))
            details.append(None)
            continue
        if fn == N.WIN_COUNT:
            vals = np.zeros(n)
        else:
            if src.type not in (D, DataType.INT64, DataType.INT32):
                raise ValueError("SUM / MIN / MAX / AVG need a numeric column")
            vals = src.data.astype(np.float64)
        value, count, absum = (frame_slices if mode == "slices" else frame_exact)(vals, src.valid, lo, hi, fn)
        if fn == N.WIN_COUNT:
            out.append(Expected(D, count.astype(np.float64), ones, False))
            details.append(None)
            continue
        details.append({"sum": value, "abs": absum, "count": count} if fn in (N.WIN_SUM, N.WIN_AVG) else None)
        if fn == N.WIN_AVG:
            with np.errstate(invalid="ignore"):
                value = value / np.maximum(count, 1)
        out.append(Expected(D, np.where(count > 0, value, 0.0), count > 0, True, None, count == 0))
    return out, details


def host_rows(cols) -> list:
    """The columns as the boxed rows ``WindowOperator``'s host branch drains."""
    return [[c.value(i) for c in cols] for i in range(len(cols[0]))]
