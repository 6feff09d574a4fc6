"""A numpy restatement of the contract of qe_result_group_ordered (include/qe_hip.h): ordered-set aggregates per group.

Pure numpy: no oracle, no GPU.  tests/test_ordered_cpu.py proves it equal to the host branch of ``OrderedAggregateOperator``
value for value; the device tests rely on that proof.

Per distinct argument column the rows are sorted (``np.lexsort``, stable) by the comparator-equivalent images of
tests/window_reference.py -- the dense rank of (validity, value) in ``compareValues`` order, NULL = 0 -- of the group columns and
then of the argument; group and run boundaries are comparisons of those ranks between neighbours.  Inside a group the NULLs stand
in front, so the valid values are ``v[k] = column[perm[first + k]]``.  The two percentile formulas are evaluated elementwise in
``np.float64``: one IEEE operation per numpy call, none fused, which is the order the header fixes.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from queryengine_amd import Column, DataType
from queryengine_amd import native as N

from window_reference import Expected, _valid, assert_window_output, key_rank  # noqa: F401 (assert_window_output: re-exported)

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
PERCENTILES = (N.OSA_PERCENTILE_CONT, N.OSA_PERCENTILE_DISC)


def entry(f) -> Tuple[int, int, float]:
    f = tuple(f)
    return int(f[0]), int(f[1]), float(f[2]) if len(f) > 2 else 0.0


def _picked(c: Column, rows: np.ndarray, have: np.ndarray) -> Expected:
    """The column gathered at `rows` where `have`, NULL (validity 0, value zero) elsewhere; always nullable."""
    rows = np.where(have, rows, 0)
    if len(c):
        data = np.where(have, c.data[rows], np.zeros(1, dtype=c.data.dtype))
        valid = have & _valid(c)[rows]
    else:
        data, valid = np.zeros(len(have), dtype=c.data.dtype), np.zeros(len(have), dtype=bool)
    return Expected(c.type, data, valid, True, c.dictionary, ~have)


def ordered_reference(cols: Sequence[Column], nullable: Sequence[bool], group_by: Sequence[int], functions: Sequence) -> Tuple[List[Expected], int]:
    """(expected output columns, groups).  `nullable[c]` = the input column carries a validity bitmap."""
    fns = [entry(f) for f in functions]
    n = len(cols[0])
    if n == 0:
        G = 0 if group_by else 1
        out = [Expected(cols[c].type, np.zeros(0, dtype=cols[c].data.dtype), np.zeros(0, dtype=bool), bool(nullable[c]), cols[c].dictionary)
               for c in group_by]
        for fn, col, _ in fns:
            if fn == N.OSA_COUNT_DISTINCT:
                out.append(Expected(D, np.zeros(G), np.ones(G, dtype=bool), False))
            elif fn == N.OSA_PERCENTILE_CONT:
                out.append(Expected(D, np.zeros(G), np.zeros(G, dtype=bool), True, None, np.ones(G, dtype=bool)))
            else:
                out.append(Expected(cols[col].type, np.zeros(G, dtype=cols[col].data.dtype), np.zeros(G, dtype=bool), True, cols[col].dictionary,
                                    np.ones(G, dtype=bool)))
        return out, G
    granks = [key_rank(cols[c]) for c in group_by]
    j = np.arange(n, dtype=np.int64)
    out: List[Expected] = []
    results = {}
    G = None
    args = list(dict.fromkeys(col for _, col, _ in fns)) or [None]
    for arg in args:
        arank = key_rank(cols[arg]) if arg is not None else np.zeros(n, dtype=np.int64)
        perm = np.lexsort(([arank] + granks[::-1])).astype(np.int64)          # last key of lexsort is the primary one
        pstart = j == 0
        for r in granks:
            s = r[perm]
            pstart = pstart | np.concatenate([[False], s[1:] != s[:-1]])
        gstart = np.nonzero(pstart)[0]
        gend = np.append(gstart[1:], n)
        gid = np.cumsum(pstart) - 1
        if G is None:
            G = len(gstart)
            for c in group_by:
                col = cols[c]
                out.append(Expected(col.type, col.data[perm[gstart]], _valid(col)[perm[gstart]], bool(nullable[c]), col.dictionary))
        assert len(gstart) == G
        if arg is None:
            break
        col = cols[arg]
        valid = _valid(col)[perm]
        c = np.bincount(gid, weights=valid, minlength=G).astype(np.int64)      # valid values of every group
        first = gend - c                                                         # NULLs sort first
        assert valid[np.minimum(first, n - 1)][c > 0].all() and not valid[np.maximum(first - 1, 0)][first > gstart].any()
        have = c > 0
        ar = arank[perm]
        prev_differs = np.concatenate([[True], (ar[1:] != ar[:-1]) | ~valid[:-1]])
        run = valid & (pstart | prev_differs)                                    # a run of equal valid values starts
        for k, (fn, fcol, q) in enumerate(fns):
            if fcol != arg:
                continue
            if fn == N.OSA_COUNT_DISTINCT:
                results[k] = Expected(D, np.bincount(gid[run], minlength=G).astype(np.float64), np.ones(G, dtype=bool), False)
            elif fn == N.OSA_PERCENTILE_DISC:
                kk = np.maximum(np.ceil(np.float64(q) * c.astype(np.float64)).astype(np.int64) - 1, 0)
                results[k] = _picked(col, perm[np.minimum(first + kk, n - 1)], have)
            elif fn == N.OSA_PERCENTILE_CONT:
                if col.type not in (D, I64, I32):
                    raise ValueError("PERCENTILE_CONT needs a numeric column")
                h = np.float64(q) * np.maximum(c - 1, 0).astype(np.float64)
                fl, ce = np.floor(h), np.ceil(h)
                frac = h - fl
                vlo = col.data[perm[np.minimum(first + fl.astype(np.int64), n - 1)]].astype(np.float64)   # converted AFTER the sort
                vhi = col.data[perm[np.minimum(first + ce.astype(np.int64), n - 1)]].astype(np.float64)
                with np.errstate(invalid="ignore", over="ignore"):
                    diff = vhi - vlo
                    step = diff * frac
                    interpolated = vlo + step
                same = (frac == 0.0) | (vlo.view(np.uint64) == vhi.view(np.uint64))
                results[k] = Expected(D, np.where(have, np.where(same, vlo, interpolated), 0.0), have, True, None, ~have)
            elif fn == N.OSA_MODE:
                rs = np.nonzero(run)[0]
                ends = np.minimum(np.append(rs[1:], n), gend[gid[rs]])
                length = ends - rs
                order = np.lexsort((rs, -length, gid[rs]))                       # per group: longest first, then earliest
                groups, at = np.unique(gid[rs][order], return_index=True)
                rows = np.zeros(G, dtype=np.int64)
                rows[groups] = perm[rs[order][at]]
                results[k] = _picked(col, rows, have)
            else:
                raise ValueError("unknown function")
    out.extend(results[k] for k in range(len(fns)))
    return out, int(G)
