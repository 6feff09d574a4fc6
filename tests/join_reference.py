"""A vectorised reference for the hash equi-join: the pairs of ``HashJoinOperator``'s host branch, and the whole expected
output as columns, in numpy -- for sides of millions of rows, which the host branch (boxed rows in Python lists) cannot serve.

Pure numpy: no oracle, no GPU.  tests/test_join_cpu.py proves it equal to the host branch, pair for pair and value for value,
on every key type, join type and edge the host branch defines; the device tests rely on that proof.

Key equality is the engine's `=`: every NaN is one value, -0.0 != 0.0 (bit images), INT32 / INT64 / BOOLEAN by
value, STRING by value across the two dictionaries (a string listed twice in a dictionary is one value), and a NULL in any
key column matches nothing.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from queryengine_amd import Column, DataType
from queryengine_amd import native as N

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
INNER, LEFT, SEMI, ANTI = N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI
CANONICAL_NAN = np.uint64(0x7ff8000000000000)


def _dense(a: np.ndarray) -> Tuple[np.ndarray, int]:
    uniq, inv = np.unique(a, return_inverse=True)
    return inv.astype(np.int64).reshape(-1), len(uniq)


def _images(pc: Column, bc: Column) -> Tuple[np.ndarray, np.ndarray]:
    """One integer per row of each side that two rows share exactly when their values are `=` (garbage under a NULL)."""
    if pc.type != bc.type:
        raise ValueError(f"key column is {pc.type.name} on the probe side and {bc.type.name} on the build side")
    if pc.type == D:
        out = []
        for c in (pc, bc):
            bits = c.data.view(np.uint64).copy()
            bits[np.isnan(c.data)] = CANONICAL_NAN
            out.append(bits)
        return out[0], out[1]
    if pc.type == S:
        ids = {s: i for i, s in enumerate(sorted(set(pc.dictionary) | set(bc.dictionary)))}
        out = []
        for c in (pc, bc):
            table = np.array([ids[s] for s in c.dictionary] + [-1], dtype=np.int64)     # (+ one entry: an empty dictionary)
            code = c.data.astype(np.int64)
            ok = (code >= 0) & (code < len(c.dictionary))
            if c.valid is not None:
                ok &= c.valid
            out.append(table[np.where(ok, code, len(c.dictionary))])
        return out[0], out[1]
    return pc.data.astype(np.int64), bc.data.astype(np.int64)


def key_ids(pcols: Sequence[Column], bcols: Sequence[Column], pk: Sequence[int], bk: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """(id per probe row, id per build row): equal ids <=> equal key tuples; -1 for a row with a NULL in a key column."""
    if not 1 <= len(pk) <= 4 or len(pk) != len(bk):
        raise ValueError("1 to 4 key columns, as many on the probe side as on the build side")
    np_, nb = len(pcols[0]), len(bcols[0])
    comb = np.zeros(np_ + nb, dtype=np.int64)
    keyed = np.ones(np_ + nb, dtype=bool)
    for cp, cb in zip(pk, bk):
        pi, bi = _images(pcols[cp], bcols[cb])
        inv, k = _dense(np.concatenate([pi, bi]))
        comb, _ = _dense(comb * k + inv)                 # dense again after every column: the product never overflows
        for c, lo in ((pcols[cp], 0), (bcols[cb], np_)):
            if c.valid is not None:
                keyed[lo:lo + len(c)] &= c.valid
    comb = np.where(keyed, comb, -1)
    return comb[:np_], comb[np_:]


def match_counts(pcols, bcols, pk, bk) -> np.ndarray:
    """Build rows that match each probe row (0 for a NULL key)."""
    pid, bid = key_ids(pcols, bcols, pk, bk)
    sids = np.sort(bid[bid >= 0])
    return np.where(pid >= 0, np.searchsorted(sids, pid, "right") - np.searchsorted(sids, pid, "left"), 0).astype(np.int64)


def reference_pairs(pcols: Sequence[Column], bcols: Sequence[Column], pk: Sequence[int], bk: Sequence[int], jt: int) -> Tuple[np.ndarray, np.ndarray]:
    """(prow, brow) as int64 arrays in nested-loop order: probe side outside, the matches of one probe row in build-row
    order; brow == -1 for the "none" of an unmatched LEFT row; brow is empty for SEMI and ANTI."""
    if jt not in (INNER, LEFT, SEMI, ANTI):
        raise ValueError("unknown join type")
    pid, bid = key_ids(pcols, bcols, pk, bk)
    n = len(pid)
    brows = np.nonzero(bid >= 0)[0]
    order = np.argsort(bid[brows], kind="stable")        # rows of one key stay in build-row order
    srows, sids = brows[order], bid[brows][order]
    lo = np.searchsorted(sids, pid, "left")
    cnt = np.where(pid >= 0, np.searchsorted(sids, pid, "right") - lo, 0).astype(np.int64)
    none = np.zeros(0, dtype=np.int64)
    if jt == SEMI:
        return np.nonzero(cnt > 0)[0].astype(np.int64), none
    if jt == ANTI:
        return np.nonzero(cnt == 0)[0].astype(np.int64), none
    out = np.maximum(cnt, 1) if jt == LEFT else cnt
    total = int(out.sum())
    prow = np.repeat(np.arange(n, dtype=np.int64), out)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(out) - out, out)
    pos = np.repeat(lo, out) + within
    matched = np.repeat(cnt > 0, out)
    brow = np.full(total, -1, dtype=np.int64)
    brow[matched] = srows[pos[matched]]
    return prow, brow


def _taken(src: Column, rows: np.ndarray, none_nulls: bool) -> Column:
    have = rows >= 0
    r = np.where(have, rows, 0)
    if len(src) == 0:                                    # nothing to take from: every row is "none"
        data = np.zeros(len(rows), dtype=src.data.dtype)
        valid = np.zeros(len(rows), dtype=bool)
    else:
        data = np.where(have, src.data[r], np.zeros(1, dtype=src.data.dtype))
        valid = (src.valid[r] if src.valid is not None else np.ones(len(rows), dtype=bool)) & have
    if not none_nulls and not have.all():
        raise ValueError('a "none" row outside the build columns of a LEFT join')
    return Column(src.type, data, valid, src.dictionary)


def expected_columns(pcols: Sequence[Column], bcols: Sequence[Column], prow: np.ndarray, brow: np.ndarray, probe_out: Sequence[int],
                     build_out: Sequence[int], jt: int) -> List[Column]:
    """The whole expected output: the listed probe columns through `prow`, then the listed build columns through `brow`.
    Validity is the source's (all valid where it has none); a "none" row of a LEFT join has validity 0 and value 0 in every
    build column.  (``Column`` drops a validity that is all ones: ``expected_nullable`` says which columns carry one.)"""
    if jt in (SEMI, ANTI) and len(build_out):
        raise ValueError("a SEMI / ANTI join has no build columns")
    out = [_taken(pcols[c], prow, False) for c in probe_out]
    out += [_taken(bcols[c], brow, jt == LEFT) for c in build_out]
    return out


def expected_nullable(probe_nullable: Sequence[bool], build_nullable: Sequence[bool], probe_out, build_out, jt: int) -> List[bool]:
    """Nullability of every output column: the source column's; under LEFT every build column is nullable."""
    return [bool(probe_nullable[c]) for c in probe_out] + [jt == LEFT or bool(build_nullable[c]) for c in build_out]


def assert_join_output(got: Sequence[Column], want: Sequence[Column], brow: Optional[np.ndarray] = None, nprobe_out: int = 0, what: str = "") -> None:
    """Every output column in full: type, dictionary, length, validity as whole arrays, data as whole arrays where valid
    (DOUBLE by bits, so NaN payloads and -0.0 count; STRING by code: both sides hold the source's dictionary).  With `brow`:
    columns from nprobe_out on are build columns, and under their "none" rows (brow == -1) the value must be zero."""
    assert len(got) == len(want), f"{what}: {len(got)} columns, want {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        name = f"{what}: column {k} ({w.type.name})"
        assert g.type == w.type, f"{name}: type {g.type.name}"
        assert g.dictionary == w.dictionary, f"{name}: dictionary differs"
        assert len(g) == len(w), f"{name}: {len(g)} rows, want {len(w)}"
        n = len(w)
        gv = g.valid if g.valid is not None else np.ones(n, dtype=bool)
        wv = w.valid if w.valid is not None else np.ones(n, dtype=bool)
        bad = np.nonzero(gv != wv)[0]
        assert bad.size == 0, f"{name}: validity differs at {bad.size} rows, first {bad[:8]} (got {gv[bad[:8]]})"
        gd, wd = (g.data.view(np.uint64), w.data.view(np.uint64)) if w.type == D else (g.data, w.data)
        bad = np.nonzero((gd != wd) & wv)[0]
        assert bad.size == 0, f"{name}: values differ at {bad.size} rows, first {bad[:8]}: got {g.data[bad[:8]]!r} want {w.data[bad[:8]]!r}"
        if brow is not None and k >= nprobe_out:
            bad = np.nonzero((brow < 0) & (gd != 0))[0]
            assert bad.size == 0, f'{name}: no zeroed value under "none" at {bad.size} rows, first {bad[:8]}: {g.data[bad[:8]]!r}'
