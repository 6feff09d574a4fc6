"""A vectorised reference for the RIGHT and FULL OUTER forms of the hash equi-join and of the range join, in numpy.

Pure numpy: no oracle, no GPU.  The output is a HEAD followed by a TAIL.  The head is today's INNER (for RIGHT) or LEFT (for
FULL) output, taken unchanged from ``join_reference.reference_pairs`` and ``range_join_reference.range_matches``.  The tail is
every build / right row that is absent from the head's build / right rows, ascending, with probe / left row -1 ("none").
tests/test_outer_join_cpu.py proves this equal to the host branches of ``HashJoinOperator`` and ``RangeJoinOperator`` row for
row; the device tests rely on that proof.

Columns: the listed probe / left columns through the first row list, then the listed build / right columns through the
second; a "none" (-1) on EITHER side has validity 0 and value zero.  Nullability follows from the schemas and the join type
alone: RIGHT makes every probe / left column nullable, FULL every column.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from queryengine_amd import Column
from queryengine_amd import native as N

from join_reference import reference_pairs
from range_join_reference import range_matches
from window_reference import Expected, _valid

RIGHT, FULL = N.JOIN_RIGHT, N.JOIN_FULL
HEAD_TYPE = {RIGHT: N.JOIN_INNER, FULL: N.JOIN_LEFT}
HASH_PROBE, RANGE_JOIN = 1, 2          # out[0] of qe_ctx_last_outer_stats


def with_tail(lrow: np.ndarray, rrow: np.ndarray, nright: int, which: int) -> Tuple[np.ndarray, np.ndarray, List[int]]:
    """(left rows, right rows, outer stats) of head + tail, from the head's two row lists (-1: none)."""
    matched = np.zeros(nright, dtype=bool)
    matched[rrow[rrow >= 0]] = True
    tail = np.nonzero(~matched)[0].astype(np.int64)
    stats = [which, len(lrow), len(tail), int(matched.sum())]
    return np.concatenate([lrow, np.full(len(tail), -1, dtype=np.int64)]), np.concatenate([rrow, tail]), stats


def hash_outer_pairs(pcols: Sequence[Column], bcols: Sequence[Column], pk: Sequence[int], bk: Sequence[int], jt: int):
    """(prow, brow, outer stats) of qe_join_probe under RIGHT / FULL; -1 = none, on either side."""
    prow, brow = reference_pairs(pcols, bcols, pk, bk, HEAD_TYPE[jt])
    return with_tail(prow, brow, len(bcols[0]), HASH_PROBE)


def range_outer_pairs(left: Sequence[Column], right: Sequence[Column], left_by, right_by, lo: int, hi: int, on: int, lo_strict: bool,
                      hi_strict: bool, jt: int):
    """(lrow, rrow, outer stats, longest) of qe_result_range_join under RIGHT / FULL; -1 = none, on either side."""
    nl = len(left[0])
    first, cnt, rlist = range_matches(left, right, left_by, right_by, lo, hi, on, lo_strict, hi_strict)
    emit = np.maximum(cnt, 1) if jt == FULL else cnt
    lrow = np.repeat(np.arange(nl, dtype=np.int64), emit)
    k = np.arange(int(emit.sum()), dtype=np.int64) - np.repeat(np.cumsum(emit) - emit, emit)
    found = cnt[lrow] > 0
    rrow = np.full(len(lrow), -1, dtype=np.int64)
    rrow[found] = rlist[first[lrow[found]] + k[found]]
    return with_tail(lrow, rrow, len(right[0]), RANGE_JOIN) + (int(cnt.max()) if nl else 0,)


def _taken(src: Column, rows: np.ndarray, nullable: bool) -> Expected:
    have = rows >= 0
    data = np.zeros(len(rows), dtype=src.data.dtype)
    valid = np.zeros(len(rows), dtype=bool)
    data[have] = src.data[rows[have]]
    valid[have] = _valid(src)[rows[have]]
    return Expected(src.type, data, valid, nullable, src.dictionary, ~have)


def outer_expected(lcols: Sequence[Column], rcols: Sequence[Column], rnullable: Sequence[bool], lrow: np.ndarray, rrow: np.ndarray,
                   left_out: Sequence[int], right_out: Sequence[int], jt: int) -> List[Expected]:
    """The whole expected output.  `rnullable[c]`: the build / right source column carries a validity bitmap (the probe / left
    columns are nullable whatever their source)."""
    assert jt in (RIGHT, FULL)
    return [_taken(lcols[c], lrow, True) for c in left_out] + [_taken(rcols[c], rrow, jt == FULL or bool(rnullable[c])) for c in right_out]
