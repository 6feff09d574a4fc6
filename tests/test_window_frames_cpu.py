"""Window frames without a GPU: ``WindowOperator``'s host branch (the executable statement of the semantics) against
tests/window_frames_reference.py, the two statements of that reference against each other, the operator's argument checks,
and the index arithmetic of the device's frame rule, exhaustively."""
import math
from fractions import Fraction

import numpy as np
import pytest

from queryengine_amd import Column, DataType
from queryengine_amd import engine as E
from queryengine_amd import native as N
from queryengine_amd.operators import Operator, WindowOperator, map as op_map

from window_frames_reference import frames_reference, host_rows

D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
UNB = N.FRAME_UNBOUNDED
SPECIALS = np.array([float("nan"), float("inf"), -float("inf"), -0.0])
FRAMES = [(0, 0), (1, 0), (0, 1), (1, 1), (3, 3), (2, 5), (7, 0), (0, 9), (40, 40), (UNB, 0), (UNB, 2), (3, UNB), (UNB, UNB), (0, UNB)]


class Rows(Operator):
    def __init__(self, rows):
        self.rows, self.i = rows, None

    def open(self):
        self.i = 0

    def close(self):
        self.i = None

    def next(self):
        if self.i >= len(self.rows):
            return None
        self.i += 1
        return self.rows[self.i - 1]


def window(cols, part, order, fns):
    return op_map(WindowOperator(Rows(host_rows(cols)), part, order, fns), list)


def columns(rng, n, fractional, special_share=0.03):
    """(partition key, order key with ties, DOUBLE values, INT64 values, nullable STRING, nullable BOOLEAN, row id)"""
    if fractional:
        vals = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 9, n)
    else:
        vals = rng.integers(-1000, 1001, n) / 2.0
        pick = rng.random(n) < special_share
        vals = np.where(pick, SPECIALS[rng.integers(0, 4, n)], vals)
    return [Column(I32, rng.integers(0, 6, n).astype(np.int32), rng.random(n) > 0.05), Column(I32, rng.integers(0, 9, n).astype(np.int32)),
            Column(D, vals, rng.random(n) > 0.15), Column(I64, rng.integers(-50, 50, n), rng.random(n) > 0.1),
            Column(S, rng.integers(0, 3, n).astype(np.int32), rng.random(n) > 0.2, ["x", "y", "zz"]), Column(B, rng.random(n) > 0.5, rng.random(n) > 0.2),
            Column(I64, np.arange(n, dtype=np.int64))]


def same(a, b):
    return a == b or (a is not None and b is not None and a != a and b != b)


def check_rows(got, want, details, fns, exact):
    ncols = len(want) - len(fns)
    assert len(got) == len(want[0].data)
    for j, row in enumerate(got):
        for k, w in enumerate(want):
            g = row[k]
            if not w.valid[j]:
                assert g is None, (j, k, g)
                continue
            assert g is not None, (j, k)
            if w.type == S:
                assert g == w.dictionary[w.data[j]]
            elif w.type != D or k < ncols:
                assert same(g, w.data[j]), (j, k, g, w.data[j])
            elif exact or details[k - ncols] is None or not math.isfinite(w.data[j]):
                assert same(float(g), float(w.data[j])) and (g != 0 or math.copysign(1, g) == math.copysign(1, w.data[j])), (j, k, g, w.data[j])
            else:      # a sequential sum of c doubles against fsum: the any-order bound, gamma_c * sum|x| (AVG: gamma_(c+1) / c)
                d = details[k - ncols]
                c, u = int(d["count"][j]), Fraction(1, 2 ** 53)
                avg = fns[k - ncols][0] == N.WIN_AVG
                m = c + 1 if avg else c
                bound = m * u / (1 - m * u) * Fraction(float(d["abs"][j])) / (c if avg else 1) + Fraction(1, 2 ** 1075)
                exact_value = Fraction(float(d["sum"][j])) / (c if avg else 1)
                assert abs(Fraction(float(g)) - exact_value) <= bound, (j, k, g, float(exact_value))


@pytest.mark.parametrize("fractional", [False, True], ids=["integer-valued", "fractional"])
def test_host_branch_equals_the_reference_row_for_row(fractional):
    rng = np.random.default_rng(41 + fractional)
    n = 260
    cols = columns(rng, n, fractional)
    nullable = [c.valid is not None for c in cols]
    for lot in range(0, len(FRAMES), 3):
        fns = []
        for p, f in FRAMES[lot:lot + 3]:
            fns += [(N.WIN_SUM, 2, 0, p, f), (N.WIN_AVG, 2, 0, p, f), (N.WIN_COUNT, 4, 0, p, f), (N.WIN_MIN, 2, 0, p, f), (N.WIN_MAX, 3, 0, p, f)]
        fns = fns[:14] + [(N.WIN_FIRST_VALUE, 4, 0) + FRAMES[lot], (N.WIN_LAST_VALUE, 5, 0) + FRAMES[lot]]
        got = window(cols, [0], [(1, True)], fns)
        want, details = frames_reference(cols, nullable, [0], [(1, True)], fns)
        check_rows(got, want, details, fns, exact=not fractional)


def test_both_statements_of_the_reference_agree():
    rng = np.random.default_rng(43)
    cols = columns(rng, 700, fractional=False, special_share=0.02)
    nullable = [c.valid is not None for c in cols]
    fns = []
    for p, f in FRAMES + [(63, 0), (100, 27)]:
        fns += [(fn, 2, 0, p, f) for fn in (N.WIN_SUM, N.WIN_COUNT, N.WIN_MIN, N.WIN_MAX, N.WIN_AVG)]
    a, da = frames_reference(cols, nullable, [0], [(1, False)], fns, "slices")
    b, db = frames_reference(cols, nullable, [0], [(1, False)], fns, "exact")
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x.valid, y.valid), k
        xv, yv = np.ascontiguousarray(x.data[x.valid]), np.ascontiguousarray(y.data[y.valid])
        if x.type == D:
            assert np.array_equal(xv.view(np.uint64)[~np.isnan(xv)], yv.view(np.uint64)[~np.isnan(yv)]) and np.array_equal(np.isnan(xv), np.isnan(yv)), k
        else:
            assert np.array_equal(xv, yv), k
    for x, y in zip(da, db):
        assert (x is None) == (y is None)
        if x is not None:
            assert np.array_equal(x["count"], y["count"]) and np.array_equal(x["abs"], y["abs"])


def test_three_tuples_behave_as_before():
    rng = np.random.default_rng(44)
    cols = columns(rng, 150, fractional=False)
    short = [(N.WIN_ROW_NUMBER,), (N.WIN_SUM, 2), (N.WIN_COUNT, 4), (N.WIN_MIN, 3), (N.WIN_AVG, 2), (N.WIN_LAG, 4, 1), (N.WIN_LEAD, 5, 2)]
    long = [(N.WIN_ROW_NUMBER, 0, 0, 0, 0), (N.WIN_SUM, 2, 0, UNB, 0), (N.WIN_COUNT, 4, 0, UNB, 0), (N.WIN_MIN, 3, 0, UNB, 0), (N.WIN_AVG, 2, 0, UNB, 0),
            (N.WIN_LAG, 4, 1, 0, 0), (N.WIN_LEAD, 5, 2, 0, 0)]
    a, b = window(cols, [0], [(1, False)], short), window(cols, [0], [(1, False)], long)
    assert len(a) == len(b) == 150 and all(all(same(x, y) for x, y in zip(r, q)) for r, q in zip(a, b))
    op = WindowOperator(Rows([]), [0], [], short)
    assert all(len(f) == 3 for f in op.functions)                     # the device call stays qe_result_window
    assert E.window_frame_fn((N.WIN_SUM, 2)) == (N.WIN_SUM, 2, 0, UNB, 0) and E.window_frame_fn((N.WIN_LAG, 1, 3)) == (N.WIN_LAG, 1, 3, 0, 0)
    assert E.window_frame_fn((N.WIN_RANK,)) == (N.WIN_RANK, 0, 0, 0, 0) and E.window_frame_fn((N.WIN_SUM, 2, 0, 3)) == (N.WIN_SUM, 2, 0, 3, 0)


def test_bad_frames_are_refused_by_the_operator():
    bad = [[(N.WIN_SUM, 0, 0, -2, 0)], [(N.WIN_SUM, 0, 0, 0, -2)], [(N.WIN_SUM, 0, 0, 2 ** 31, 0)], [(N.WIN_MAX, 0, 0, 0, 2 ** 31)],
           [(N.WIN_ROW_NUMBER, 0, 0, 1, 0)], [(N.WIN_RANK, 0, 0, 0, 1)], [(N.WIN_DENSE_RANK, 0, 0, UNB, 0)], [(N.WIN_LAG, 0, 1, 1, 1)],
           [(N.WIN_LEAD, 0, 1, UNB, UNB)], [(12, 0, 0, 0, 0)], [(N.WIN_FIRST_VALUE, 0)], [(N.WIN_LAST_VALUE, 0, 0)]]
    for fns in bad:
        with pytest.raises(ValueError):
            WindowOperator(Rows([]), [0], [], fns)
    WindowOperator(Rows([]), [0], [], [(N.WIN_FIRST_VALUE, 0, 0, UNB, UNB), (N.WIN_SUM, 0, 0, 2 ** 31 - 1, 2 ** 31 - 1)])
    with pytest.raises(ValueError):
        window([Column.from_values(I32, [1]), Column.from_values(S, ["a"])], [0], [], [(N.WIN_SUM, 1, 0, 1, 1)])


def test_null_arguments_are_refused_without_a_device():
    ctx = E.Context(device=None)
    try:
        fns = (N.WindowFrameFn * 1)(N.WindowFrameFn(N.WIN_SUM, 0, 0, 1, 1))
        out = E.C.c_void_p(0xdead)
        fake = E.C.c_void_p(0)          # a null result is refused before the device is asked for
        assert ctx._lib.qe_result_window_frames(ctx.handle, fake, None, 0, None, 0, fns, 1, E.C.byref(out)) == 1 and out.value is None
    finally:
        ctx.close()


# ---- the device's frame rule (win_frame_kernel), restated ------------------------------------------------------------------------
def test_the_block_rule_covers_every_frame_exactly():
    """P[h] (forward scan restarted at partition and block starts) holds rows max(h - h % W, start) .. h; S[l] (reverse scan
    restarted at partition and block ends) holds rows l .. min(l - l % W + W - 1, end).  For every partition [start, end] with
    end < 40, every row j and every (p, f) -- p, f >= 40 clamp like 40 and W > 40 puts one block over all rows, so 0 .. 41
    is every behaviour -- the piece or the two pieces the rule picks are exactly [lo, hi]: contiguous, disjoint, nothing
    outside."""
    p, f = np.meshgrid(np.arange(42), np.arange(42), indexing="ij")
    W = p + f + 1
    cases = 0
    for start in range(40):
        for end in range(start, 40):
            for j in range(start, end + 1):
                lo, hi = np.maximum(start, j - p), np.minimum(end, j + f)
                assert (lo <= j).all() and (j <= hi).all() and (hi - lo + 1 <= W).all()
                p_from = np.maximum(hi - hi % W, start)            # first row of P[hi]
                s_to = np.minimum(lo - lo % W + W - 1, end)        # last row of S[lo]
                one = p_from == lo                                 # case 1: P[hi] alone
                two = ~one & (s_to == hi)                          # case 2: S[lo] alone
                both = ~one & ~two                                 # case 3: S[lo] then P[hi]
                assert (s_to[both] + 1 == p_from[both]).all(), (start, end, j)
                assert (lo[both] <= s_to[both]).all() and (p_from[both] <= hi[both]).all(), (start, end, j)
                cases += W.size
    assert cases == 42 * 42 * sum(end - start + 1 for start in range(40) for end in range(start, 40))
