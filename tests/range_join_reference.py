"""A vectorised reference for the range join: the rows of ``RangeJoinOperator``'s host branch as columns, in numpy -- for inputs
of hundreds of thousands of rows and outputs of millions, which the host branch (a nested loop over boxed rows) cannot serve.

Pure numpy: no oracle, no GPU.  tests/test_range_join_cpu.py proves it equal to the host branch row for row; the device tests
rely on that proof.

The by columns are ranked over BOTH sides at once with ``window_reference.key_rank`` (NULL = 0; DOUBLE in ``Double.compareTo``
order with every NaN one value and -0.0 below 0.0; STRING by string, through the merged dictionary of
``setop_reference.concatenated``) and fold into one partition id.  ``lo``, ``hi`` and ``on`` are ranked TOGETHER in one
``key_rank`` call, so that the three are comparable (INT64 as int64, never through a double), and (partition id, value rank)
folds into one int64 key whose order is (partition, value).  The eligible right rows -- every by column and ``on`` valid --
are ordered by ``np.lexsort`` on (partition, on, row); every eligible left row -- every by column, ``lo`` and ``hi`` valid --
does two ``np.searchsorted`` calls in their keys:

    first   the right keys below lo: side="left"; a strict lower end also skips those equal to it: side="right"
    end     the right keys up to hi: side="right"; a strict upper end stops before those equal to it: side="left"

Its matches are the rows of that list in [first, end): none when end <= first (an empty or reversed interval).  A key of
another partition lies below both keys of a left row or above both, so it is never counted.  ``np.repeat`` expands the counts.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from queryengine_amd import Column
from queryengine_amd import native as N

from setop_reference import concatenated
from window_reference import Expected, _valid, key_rank


def range_matches(left: Sequence[Column], right: Sequence[Column], left_by: Sequence[int], right_by: Sequence[int], left_lo: int,
                  left_hi: int, right_on: int, lo_strict: bool, hi_strict: bool) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(first, cnt, rlist): the matches of left row l are the right rows rlist[first[l] : first[l] + cnt[l]], in output order."""
    nl, nr = len(left[0]), len(right[0])
    first, cnt = np.zeros(nl, dtype=np.int64), np.zeros(nl, dtype=np.int64)
    if nl == 0 or nr == 0:
        return first, cnt, np.zeros(0, dtype=np.int64)
    n = nl + nr
    cat, _ = concatenated([left[c] for c in left_by], [right[c] for c in right_by])
    whole = np.ones(n, dtype=bool)                           # no NULL in any by column
    for c in cat:
        whole &= _valid(c)
    if cat:
        _, part = np.unique(np.stack([key_rank(c) for c in cat], axis=1), axis=0, return_inverse=True)
        part = part.reshape(-1).astype(np.int64)             # over both sides: rows 0 .. nl - 1 are the left's
    else:
        part = np.zeros(n, dtype=np.int64)
    lo, hi, on = left[left_lo], left[left_hi], right[right_on]
    assert lo.type == hi.type == on.type
    values = Column(lo.type, np.concatenate([lo.data, hi.data, on.data]), np.concatenate([_valid(lo), _valid(hi), _valid(on)]))
    rank = key_rank(values)                                  # ONE ranking: lo, hi and on are comparable
    width = int(rank.max()) + 1
    lo_key, hi_key = part[:nl] * width + rank[:nl], part[:nl] * width + rank[nl:2 * nl]
    lok = whole[:nl] & _valid(lo) & _valid(hi)
    rrow = np.nonzero(whole[nl:] & _valid(on))[0]
    rpart, ron = part[nl:][rrow], rank[2 * nl:][rrow]
    order = np.lexsort((rrow, ron, rpart))                   # by (partition, on), ties in right row order
    rlist, rkey = rrow[order], (rpart * width + ron)[order]
    begin = np.searchsorted(rkey, lo_key, side="right" if lo_strict else "left")
    end = np.searchsorted(rkey, hi_key, side="left" if hi_strict else "right")
    cnt = np.where(lok, np.maximum(end - begin, 0), 0).astype(np.int64)
    first = np.where(cnt > 0, begin, 0).astype(np.int64)
    return first, cnt, rlist.astype(np.int64)


def range_reference(left: Sequence[Column], right: Sequence[Column], left_nullable: Sequence[bool], right_nullable: Sequence[bool],
                    left_by: Sequence[int], right_by: Sequence[int], left_lo: int, left_hi: int, right_on: int, lo_strict: bool,
                    hi_strict: bool, join_type: int, left_out: Sequence[int], right_out: Sequence[int]) -> Tuple[List[Expected], dict]:
    """(expected output columns, expected last_range_stats).  `*_nullable[c]` = that side's column carries a validity bitmap
    (``Column`` drops one that is all ones)."""
    nl, nr = len(left[0]), len(right[0])
    first, cnt, rlist = range_matches(left, right, left_by, right_by, left_lo, left_hi, right_on, lo_strict, hi_strict)
    if join_type == N.JOIN_SEMI:
        lrows, theirs = np.nonzero(cnt > 0)[0], None
    elif join_type == N.JOIN_ANTI:
        lrows, theirs = np.nonzero(cnt == 0)[0], None
    else:
        emit = np.maximum(cnt, 1) if join_type == N.JOIN_LEFT else cnt
        lrows = np.repeat(np.arange(nl, dtype=np.int64), emit)
        k = np.arange(int(emit.sum()), dtype=np.int64) - np.repeat(np.cumsum(emit) - emit, emit)
        found = cnt[lrows] > 0
        theirs = np.full(len(lrows), -1, dtype=np.int64)
        theirs[found] = rlist[first[lrows[found]] + k[found]]
    stats = {"left_rows": nl, "right_rows": nr, "output_rows": len(lrows), "longest": int(cnt.max()) if nl else 0}
    out = []
    for c in left_out:
        col = left[c]
        out.append(Expected(col.type, col.data[lrows], _valid(col)[lrows], bool(left_nullable[c]), col.dictionary))
    for c in right_out:
        col = right[c]
        found = theirs >= 0
        data = np.zeros(len(lrows), dtype=col.data.dtype)
        valid = np.zeros(len(lrows), dtype=bool)
        data[found] = col.data[theirs[found]]
        valid[found] = _valid(col)[theirs[found]]
        out.append(Expected(col.type, data, valid, bool(right_nullable[c]) or join_type == N.JOIN_LEFT, col.dictionary, ~found))
    return out, stats
