"""A vectorised reference for the ASOF join: the rows of ``AsofJoinOperator``'s host branch as columns, in numpy -- for inputs
of hundreds of thousands of rows, which the host branch (a nested loop over boxed rows) cannot serve.

Pure numpy: no oracle, no GPU.  tests/test_asof_cpu.py proves it equal to the host branch row for row; the device tests rely
on that proof.

Every key column is ranked over BOTH sides at once with ``window_reference.key_rank`` (NULL = 0; DOUBLE in ``Double.compareTo``
order with every NaN one value and -0.0 below 0.0; STRING by string, through the merged dictionary of
``setop_reference.concatenated``; INT64 as int64, never through a double).  The by ranks of a row fold into one partition id,
and (partition id, rank of ``on``) into one int64 key whose order is (partition, on).  The eligible right rows -- every by
column and ``on`` valid -- are sorted by that key with ``np.lexsort``, ties in right row order, and every eligible left row
does one ``np.searchsorted`` in them:

    BACKWARD, not strict   the LAST right key <= mine: side="right", minus one -- of equal keys the greatest right row
    BACKWARD, strict       the last right key <  mine: side="left", minus one
    FORWARD,  not strict   the FIRST right key >= mine: side="left" -- of equal keys the smallest right row
    FORWARD,  strict       the first right key >  mine: side="right"

and the hit counts only when it lies in the same partition.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from queryengine_amd import Column
from queryengine_amd import native as N

from setop_reference import concatenated
from window_reference import Expected, _valid, key_rank


def asof_matches(left: Sequence[Column], right: Sequence[Column], left_by: Sequence[int], right_by: Sequence[int], left_on: int,
                 right_on: int, direction: int, strict: bool) -> Tuple[np.ndarray, int]:
    """(match, partitions): match[l] = the right row of left row l or -1; partitions = distinct by tuples over both sides, NULL
    counting as a value (0 when there are no rows at all)."""
    nl, nr = len(left[0]), len(right[0])
    n = nl + nr
    match = np.full(nl, -1, dtype=np.int64)
    if n == 0:
        return match, 0
    lkeys = [left[c] for c in left_by] + [left[left_on]]
    rkeys = [right[c] for c in right_by] + [right[right_on]]
    cat, _ = concatenated(lkeys, rkeys)
    ranks = [key_rank(c) for c in cat]                      # over both sides: rows 0 .. nl - 1 are the left's
    eligible = np.ones(n, dtype=bool)
    for c in cat:
        eligible &= _valid(c)
    if len(ranks) > 1:
        _, part = np.unique(np.stack(ranks[:-1], axis=1), axis=0, return_inverse=True)
        part = part.reshape(-1).astype(np.int64)
    else:
        part = np.zeros(n, dtype=np.int64)
    partitions = int(part.max()) + 1
    on = ranks[-1]
    width = int(on.max()) + 1
    key = part * width + on                                 # order = (partition, on)
    lrow = np.nonzero(eligible[:nl])[0]
    rrow = np.nonzero(eligible[nl:])[0]
    if len(lrow) == 0 or len(rrow) == 0:
        return match, partitions
    rkey = key[nl + rrow]
    order = np.lexsort((rrow, rkey))                        # by key, ties in right row order
    rkey, rrow = rkey[order], rrow[order]
    mine = key[lrow]
    if direction == N.ASOF_BACKWARD:
        at = np.searchsorted(rkey, mine, side="left" if strict else "right") - 1
    else:
        at = np.searchsorted(rkey, mine, side="right" if strict else "left")
    inside = (at >= 0) & (at < len(rkey))
    at = np.where(inside, at, 0)
    hit = inside & (rkey[at] // width == part[lrow])        # never across a partition
    match[lrow[hit]] = rrow[at[hit]]
    return match, partitions


def asof_reference(left: Sequence[Column], right: Sequence[Column], left_nullable: Sequence[bool], right_nullable: Sequence[bool],
                   left_by: Sequence[int], right_by: Sequence[int], left_on: int, right_on: int, direction: int, strict: bool,
                   join_type: int, left_out: Sequence[int], right_out: Sequence[int]) -> Tuple[List[Expected], dict]:
    """(expected output columns, expected last_asof_stats).  `*_nullable[c]` = that side's column carries a validity bitmap
    (``Column`` drops one that is all ones)."""
    nl, nr = len(left[0]), len(right[0])
    match, partitions = asof_matches(left, right, left_by, right_by, left_on, right_on, direction, strict)
    stats = {"left_rows": nl, "right_rows": nr, "matched": int((match >= 0).sum()), "partitions": partitions}
    lrows = np.arange(nl, dtype=np.int64) if join_type == N.JOIN_LEFT else np.nonzero(match >= 0)[0]
    theirs = match[lrows]
    found = theirs >= 0
    out = []
    for c in left_out:
        col = left[c]
        out.append(Expected(col.type, col.data[lrows], _valid(col)[lrows], bool(left_nullable[c]), col.dictionary))
    for c in right_out:
        col = right[c]
        data = np.zeros(len(lrows), dtype=col.data.dtype)
        valid = np.zeros(len(lrows), dtype=bool)
        data[found] = col.data[theirs[found]]
        valid[found] = _valid(col)[theirs[found]]
        out.append(Expected(col.type, data, valid, bool(right_nullable[c]) or join_type == N.JOIN_LEFT, col.dictionary, ~found))
    return out, stats
