"""A vectorised reference for the set operations: the rows of ``SetOperator``'s host branch as columns, in numpy -- for inputs
of hundreds of thousands of rows, which the host branch (boxed rows in Python lists) cannot serve.

Pure numpy: no oracle, no GPU.  tests/test_setop_cpu.py proves it equal to the host branch row for row; the device tests rely
on that proof.

The two column lists are concatenated, left rows first; a STRING column whose sides carry different dictionaries gets the
merged dictionary of the contract (left entries, then the right entries the left does not hold, in the right's order) and the
right codes go through the translation table.  The sort is ``np.lexsort`` (stable) over ``window_reference.key_rank`` images
of every column, tuple boundaries compare those ranks between neighbours, cL and cR are per-tuple counts, and a row is kept
when it is among the first k rows of its tuple.  The value under a NULL is whatever the source row held: ``zero_at`` stays
unset.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from queryengine_amd import Column
from queryengine_amd import native as N

from window_reference import Expected, S, _valid, key_rank


def merged_dictionary(left: Sequence[str], right: Sequence[str]) -> Tuple[List[str], np.ndarray]:
    """(merged entries, table right code -> merged code): the left entries unchanged, then every right entry the left does not
    hold, in the right's order; a right entry the left holds maps to its FIRST code on the left."""
    entries = list(left)
    first = {}
    for i, s in enumerate(left):
        first.setdefault(s, i)
    table = np.zeros(len(right), dtype=np.int32)
    for i, s in enumerate(right):
        if s in first:
            table[i] = first[s]
        else:
            table[i] = len(entries)
            entries.append(s)
    return entries, table


def kept_copies(op: int, all: bool, cl: np.ndarray, cr: np.ndarray) -> np.ndarray:   # noqa: A002
    if op == N.SET_UNION:
        return cl + cr if all else np.ones_like(cl)
    if op == N.SET_INTERSECT:
        return np.minimum(cl, cr) if all else ((cl > 0) & (cr > 0)).astype(np.int64)
    return np.maximum(cl - cr, 0) if all else ((cl > 0) & (cr == 0)).astype(np.int64)


def concatenated(left: Sequence[Column], right: Sequence[Column], shared: Optional[Sequence[bool]] = None) -> Tuple[List[Column], int]:
    """(the columns of left rows then right rows, STRING columns translated; STRING columns that were translated).  shared[c]:
    both sides carry ONE dictionary object (default: their entry lists are equal, which is what one context makes of them)."""
    cols, translated = [], 0
    for c, (l, r) in enumerate(zip(left, right)):
        assert l.type == r.type
        rdata, dictionary = r.data, l.dictionary
        if l.type == S and not (l.dictionary == r.dictionary if shared is None else shared[c]):
            dictionary, table = merged_dictionary(l.dictionary, r.dictionary)
            in_range = (r.data >= 0) & (r.data < len(r.dictionary))
            rdata = np.where(in_range, table[np.where(in_range, r.data, 0)] if len(table) else 0, 0).astype(np.int32)
            translated += 1
        cols.append(Column(l.type, np.concatenate([l.data, rdata]), np.concatenate([_valid(l), _valid(r)]), dictionary))
    return cols, translated


class Analysis:
    """What every form of one (left, right) pair shares: the concatenation, its stable sort, the tuples and their counts."""

    def __init__(self, left: Sequence[Column], right: Sequence[Column], shared: Optional[Sequence[bool]] = None):
        self.nl, self.nr = len(left[0]), len(right[0])
        self.cat, self.translated = concatenated(left, right, shared)
        n = self.n = self.nl + self.nr
        if n == 0:
            return
        ranks = [key_rank(c) for c in self.cat]
        self.perm = np.lexsort(ranks[::-1]).astype(np.int64)
        start = np.zeros(n, dtype=bool)
        start[0] = True
        for r in ranks:
            s = r[self.perm]
            start[1:] |= s[1:] != s[:-1]
        self.tid = np.cumsum(start) - 1
        self.first = np.nonzero(start)[0]
        self.size = np.bincount(self.tid)
        self.cl = np.bincount(self.tid, weights=(self.perm < self.nl)).astype(np.int64)


def setop_reference(left: Sequence[Column], right: Sequence[Column], left_nullable: Sequence[bool], right_nullable: Sequence[bool],
                    op: int, all: bool = False, shared: Optional[Sequence[bool]] = None,   # noqa: A002
                    analysis: Optional[Analysis] = None) -> Tuple[List[Expected], dict]:
    """(expected output columns, expected last_set_stats).  `*_nullable[c]` = that side's column carries a validity bitmap
    (``Column`` drops one that is all ones).  `analysis`: an ``Analysis`` of the same pair, computed once for several forms."""
    a = analysis if analysis is not None else Analysis(left, right, shared)
    nullable = [bool(x) or bool(y) for x, y in zip(left_nullable, right_nullable)]
    stats = {"left_rows": a.nl, "right_rows": a.nr, "tuples": 0, "translated_columns": a.translated}
    if op == N.SET_UNION and all:
        rows = np.arange(a.n, dtype=np.int64)
    elif a.n == 0:
        rows = np.zeros(0, dtype=np.int64)
    else:
        k = kept_copies(op, all, a.cl, a.size - a.cl)
        keep = (np.arange(a.n) - a.first[a.tid]) < k[a.tid]
        rows = a.perm[keep]
        stats["tuples"] = int(len(a.first))
    out = [Expected(c.type, c.data[rows], _valid(c)[rows], nl_, c.dictionary) for c, nl_ in zip(a.cat, nullable)]
    return out, stats
