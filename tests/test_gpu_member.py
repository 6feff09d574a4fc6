"""IN and LIKE on the GPU, in every execution form (any_ctx), bit-exact against member_reference.py (numpy restatements of the
two functions, the CPU oracle for everything around them).  Every case's columns and expectation are made once and shared by
the five forms."""
import numpy as np
import pytest

from queryengine_amd import AggregationFunction as AF
from queryengine_amd import Column
from queryengine_amd import engine as E

from helpers import B, D, I32, I64, S, Fn, _rows_equal, assert_columns_equal, col, fn, num, random_column
from member_reference import expected_filter_project, in_, like, lower

pytestmark = pytest.mark.gpu

RAGGED = [0, 1, 63, 64, 65, 129, 513, 16385, 70001]   # word, tile and chunk boundaries
PATTERNS = ["random20", "all_null", "bitmap_no_null", "no_bitmap", "alternating_words"]
SPAN = 1 << 20                                        # QE_IN_BITS_SPAN's default: a bit table covers spans below it
NAN = float("nan")
TWO53 = 2 ** 53

NARROW = [100 + 3 * k for k in range(33)]                                  # bit table: span 96
WIDE = [k * 1000003 - 17000000 for k in range(30)] + [TWO53 + 2, TWO53 + 4, -(TWO53 + 2)]   # hash; three beyond 2^53
DOUBLES = [k + 0.5 for k in range(30)] + [NAN, 0.0, -0.0]                  # hash on canonical images
DICT5000 = ["name %04d" % i for i in range(5000)]


def validity(pattern: str, n: int, rng) -> np.ndarray:
    if pattern == "random20":
        return rng.random(n) >= 0.2
    if pattern == "all_null":
        return np.zeros(n, dtype=bool)
    if pattern in ("bitmap_no_null", "no_bitmap"):
        return np.ones(n, dtype=bool)
    i = np.arange(n)   # 64-row words alternately all-NULL and all-valid, with bits 0 / 63 of some words flipped
    w = i // 64
    v = (w % 2) == 1
    flip = ((i % 64 == 0) & np.isin(w % 4, (0, 1))) | ((i % 64 == 63) & np.isin(w % 4, (1, 2)))
    return v ^ flip


def with_validity(c: Column, pattern: str, rng, garbage=None) -> Column:
    """`c` with the pattern's validity.  `garbage`: values written under the NULLs -- codes outside the dictionary, integers
    far outside a bit table's span: a NULL row must neither match nor read out of bounds."""
    n = len(c)
    valid = None if pattern == "no_bitmap" else validity(pattern, n, rng)
    data = c.data.copy()
    if garbage is not None and valid is not None and n:
        nulls = np.nonzero(~valid)[0]
        data[nulls] = np.resize(np.array(garbage, dtype=data.dtype), nulls.size)
    out = Column(c.type, data, valid, c.dictionary)
    if pattern == "bitmap_no_null" and n:
        out.valid = np.ones(n, dtype=bool)
    return out


CODE_GARBAGE = [5000, -1, 2 ** 31 - 1, -(2 ** 31), 123456789, 5001]
INT_GARBAGE = [2 ** 62, -(2 ** 62), 2 ** 63 - 1, -(2 ** 63), 100 + 2 ** 32, 100 - 2 ** 32, 100 + SPAN, 99]


def run(ctx, cols, flt, projs, want):
    batch = E.DeviceBatch.from_columns(ctx, cols)
    res = E.filter_project(ctx, batch, ctx.compile(flt) if flt is not None else None, [ctx.compile(p) for p in projs])
    try:
        got = res.to_columns()
        assert res.count == len(want[0])
        for i, (g, w) in enumerate(zip(got, want)):
            assert_columns_equal(g, w, f"projection {i}")
    finally:
        res.free()
        batch.free()
    return got


_cache = {}


def shared(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def case(oracle, cols, flt, projs):
    return cols, flt, projs, expected_filter_project(oracle, cols, flt, projs)


def int_values(rng, n, members, lo, hi, dtype=np.int64):
    """Half of the rows members of the list, the rest uniform in [lo, hi)."""
    v = rng.integers(lo, hi, n).astype(dtype)
    pick = rng.random(n) < 0.5
    v[pick] = rng.choice(np.array(members, dtype=dtype), int(pick.sum()))
    return v


# ---- 1. one plan per route at the ragged sizes ------------------------------------------------------------------------
def _route_cases(oracle, n):
    rng = np.random.default_rng(4000 + n)
    a = with_validity(Column(I64, int_values(rng, n, NARROW, 80, 220)), "random20", rng, INT_GARBAGE)
    w = with_validity(Column(I64, int_values(rng, n, WIDE + [TWO53 + 1, TWO53 + 3, TWO53 + 5], -(2 ** 40), 2 ** 40)), "random20", rng)
    c = with_validity(Column(D, rng.choice(np.array(DOUBLES + [1.0, 2.25, -7.5, float("inf")]), n)), "random20", rng)
    s = with_validity(Column(S, rng.integers(0, 5000, n, dtype=np.int32), None, DICT5000), "random20", rng, CODE_GARBAGE)
    b = Column(I64, np.arange(n, dtype=np.int64))
    cols = [a, w, c, s, b]
    A_, W_, C_, S_, B_ = col("a", 0, I64), col("w", 1, I64), col("c", 2, D), col("s", 3, S), col("b", 4, I64)
    return [case(oracle, cols, in_(A_, [103, 106]), [B_]),                        # chain
            case(oracle, cols, in_(A_, NARROW), [B_]),                            # bit table
            case(oracle, cols, in_(W_, WIDE), [B_, W_]),                          # hash set on the double images (|L| >= 2^53)
            case(oracle, cols, in_(C_, DOUBLES), [B_, C_]),                       # hash set on canonical images
            case(oracle, cols, in_(S_, DICT5000[100:140]), [B_])]                 # bit per dictionary code


@pytest.mark.parametrize("n", RAGGED)
def test_routes_at_ragged_sizes(any_ctx, oracle, n):
    cases = shared(("routes", n), lambda: _route_cases(oracle, n))
    for cols, flt, projs, want in cases:
        run(any_ctx, cols, flt, projs, want)
    if n >= 513:
        assert all(0 < len(want[0]) < n for _, _, _, want in cases)


# ---- 2. validity patterns with garbage under the NULLs ----------------------------------------------------------------
def _pattern_cases(oracle):
    n = 4001
    rng = np.random.default_rng(41)
    out = []
    for pattern in PATTERNS:
        a = with_validity(Column(I64, int_values(rng, n, NARROW, 80, 220)), pattern, rng, INT_GARBAGE)
        i = with_validity(Column(I32, int_values(rng, n, NARROW, 80, 220, np.int32)), pattern, rng, [2 ** 31 - 1, -(2 ** 31), 99, 197])
        w = with_validity(Column(I64, int_values(rng, n, WIDE[:30], -(2 ** 40), 2 ** 40)), pattern, rng, INT_GARBAGE)
        s = with_validity(Column(S, rng.integers(0, 5000, n, dtype=np.int32), None, DICT5000), pattern, rng, CODE_GARBAGE)
        A_, I_, W_, S_ = col("a", 0, I64), col("i", 1, I32), col("w", 2, I64), col("s", 3, S)
        projs = [in_(A_, NARROW), in_(I_, NARROW), in_(W_, WIDE[:30] + [5, 6, 7]), in_(S_, DICT5000[100:140]), like(S_, "name 1_3%"),
                 in_(A_, [103, 106])]
        out.append((pattern, case(oracle, [a, i, w, s], None, projs)))
        out.append((pattern, case(oracle, [a, i, w, s], fn(Fn.AND, in_(A_, NARROW), in_(S_, DICT5000[0:2500])), [I_])))
    return out


def test_validity_patterns(any_ctx, oracle):
    """The result is NULL exactly where the value is; under the NULLs stand codes >= the dictionary size and negative ones, and
    integers far outside the bit table's span."""
    for pattern, (cols, flt, projs, want) in shared("patterns", lambda: _pattern_cases(oracle)):
        got = run(any_ctx, cols, flt, projs, want)
        if flt is None:
            for g, src in zip(got, (0, 1, 2, 3, 3, 0)):
                ones = np.ones(len(g), dtype=bool)
                assert np.array_equal(ones if g.valid is None else g.valid, ones if cols[src].valid is None else cols[src].valid)
        elif pattern == "all_null":
            assert len(want[0]) == 0


# ---- 3. numeric list shapes -------------------------------------------------------------------------------------------
def _numeric_cases(oracle):
    n = 4001
    rng = np.random.default_rng(43)
    near = [100, 101, 99, 100 + SPAN - 3, 100 + SPAN - 2, 100 + SPAN - 1, 100 + SPAN, 100 + SPAN + 1, 196, 197, 103]
    a = Column(I64, np.concatenate([np.array(near, dtype=np.int64), int_values(rng, n - len(near), NARROW + near, 80, 220)]), rng.random(n) >= 0.1)
    i = Column(I32, a.data.astype(np.int32), rng.random(n) >= 0.1)
    beyond = [TWO53, TWO53 + 1, TWO53 + 2, TWO53 + 3, TWO53 - 1, -TWO53, -TWO53 - 1, -TWO53 - 2, 2 ** 63 - 1, -(2 ** 63)]
    w = Column(I64, np.concatenate([np.array(beyond, dtype=np.int64), int_values(rng, n - len(beyond), WIDE + beyond, -(2 ** 40), 2 ** 40)]),
               rng.random(n) >= 0.1)
    specials = [0.0, -0.0, NAN, -NAN, 0.5, 1.5, float("inf"), float("-inf"), 5e-324, 29.5]
    c = Column(D, np.concatenate([np.array(specials), rng.choice(np.array(DOUBLES + [1.0, 2.25]), n - len(specials))]), rng.random(n) >= 0.1)
    A_, I_, W_, C_ = col("a", 0, I64), col("i", 1, I32), col("w", 2, I64), col("c", 3, D)
    cols = [a, i, w, c]
    edge = lambda span: NARROW + [100 + span]   # noqa: E731 -- 34 members whose span is `span`
    return [
        # sizes 1, 2, 33 of narrow integers; literals that no integer equals (a fraction, -0.0, NaN, +-Inf) beside them
        case(oracle, cols, None, [in_(A_, [103]), in_(A_, [103, 196]), in_(A_, NARROW), in_(A_, [103, 103.5, -0.0, NAN, float("inf")]),
                                  in_(I_, NARROW), in_(I_, [103, float(2 ** 31), -float(2 ** 31) - 1]), in_(A_, [0.5, NAN])]),
        # the span at the table's edge: S - 2 and S - 1 are bit tables, S is a hash set
        case(oracle, cols, None, [in_(A_, edge(SPAN - 2)), in_(A_, edge(SPAN - 1)), in_(A_, edge(SPAN)), in_(I_, edge(SPAN - 1))]),
        # hash sets: 33 DOUBLEs with NaN and both zeros; 33 wide INT64 with values beyond 2^53 and their double neighbours in the
        # column (2^53 + 1 converts to 2^53: it IS in a list that holds 2^53); wide integers below 2^53 (on the integers)
        case(oracle, cols, None, [in_(C_, DOUBLES), in_(W_, WIDE), in_(W_, WIDE[:30] + [TWO53, -TWO53, 1]), in_(W_, WIDE[:30] + [1, 2, 3]),
                                  in_(C_, [0.0]), in_(C_, [-0.0, NAN])]),
        case(oracle, cols, in_(W_, WIDE[:30] + [TWO53, -TWO53, 1]), [W_, in_(C_, DOUBLES)]),
    ]


def test_numeric_list_shapes(any_ctx, oracle):
    cases = shared("numeric", lambda: _numeric_cases(oracle))
    for cols, flt, projs, want in cases:
        run(any_ctx, cols, flt, projs, want)
    edge = cases[1][3]
    valid = cases[1][0][0].valid
    rows = {v: k for k, v in enumerate(cases[1][0][0].data[:11].tolist())}
    for proj, span in ((0, SPAN - 2), (1, SPAN - 1), (2, SPAN)):
        for v in (100 + SPAN - 2, 100 + SPAN - 1, 100 + SPAN):
            if valid[rows[v]]:
                assert bool(edge[proj].data[rows[v]]) == (v == 100 + span)
    big = cases[2][3][2]                                                       # w IN (.., 2^53, -2^53, 1)
    wv = cases[2][0][2]
    for k, v in enumerate(wv.data[:10].tolist()):
        if wv.valid[k]:
            assert bool(big.data[k]) == (v in (TWO53, TWO53 + 1, -TWO53, -TWO53 - 1)), v


def _cap_case(oracle):
    n = 4001
    rng = np.random.default_rng(47)
    members = (np.arange(65536, dtype=np.int64) * 2654435761) % (2 ** 45) - 2 ** 44      # 65 536 distinct wide integers
    assert len(set(members.tolist())) == 65536
    v = rng.integers(-(2 ** 44), 2 ** 44, n)
    pick = rng.random(n) < 0.5
    v[pick] = rng.choice(members, int(pick.sum()))
    a = Column(I64, v, rng.random(n) >= 0.1)
    A_ = col("a", 0, I64)
    return case(oracle, [a], in_(A_, members.tolist()), [A_])


def test_hash_set_at_the_cap(any_ctx, oracle):
    cols, flt, projs, want = shared("cap", lambda: _cap_case(oracle))
    run(any_ctx, cols, flt, projs, want)
    assert 1000 < len(want[0]) < 3000


def _collision_case(oracle):
    n = 4001
    rng = np.random.default_rng(53)
    members = [k * 7919 + 11 for k in range(48)]                                           # a list no other test uses: the plan is new
    a = Column(I64, int_values(rng, n, members + [m + 1 for m in members], 0, 400000), rng.random(n) >= 0.1)
    c = Column(D, a.data.astype(np.float64) + 0.25, a.valid)
    A_, C_ = col("a", 0, I64), col("c", 1, D)
    return case(oracle, [a, c], in_(A_, members), [A_, in_(C_, [m + 0.25 for m in members])])


def test_collisions_under_two_hash_bits(any_ctx, oracle, monkeypatch):
    """QE_IN_HASH_BITS=2: 48 literals share four home slots, only the comparison of the full image keeps them apart."""
    monkeypatch.setenv("QE_IN_HASH_BITS", "2")
    cols, flt, projs, want = shared("collisions", lambda: _collision_case(oracle))
    run(any_ctx, cols, flt, projs, want)
    assert 500 < len(want[0]) < 3500


# ---- 4. STRING --------------------------------------------------------------------------------------------------------
def _string_cases(oracle):
    n = 4001
    rng = np.random.default_rng(59)
    s = with_validity(Column(S, rng.integers(0, 5000, n, dtype=np.int32), None, DICT5000), "random20", rng, CODE_GARBAGE)
    s.data[:8] = [7, 100, 139, 140, 99, 4999, 0, 2500]
    b = Column(I64, np.arange(n, dtype=np.int64))
    S_, B_ = col("s", 0, S), col("b", 1, I64)
    absent = ["absent", "name 5000", "", "NAME 0007"]
    lists = [absent, [DICT5000[7]] + absent, [DICT5000[7], DICT5000[2500], DICT5000[4999], "absent"], DICT5000[100:140] + absent, DICT5000]
    cols = [s, b]
    return [case(oracle, cols, None, [in_(S_, l) for l in lists] + [fn(Fn.NOT, in_(S_, lists[3]))]),
            case(oracle, cols, in_(S_, lists[2]), [B_, S_]),
            case(oracle, cols, in_(S_, lists[4]), [B_]),                                   # every entry: the validity alone
            case(oracle, cols, in_(S_, lists[0]), [B_])]                                   # no entry: keeps nothing


def test_string_in(any_ctx, oracle):
    """A 5000-entry dictionary; lists selecting 0, 1, 3, 40 and all entries, each with literals absent from the dictionary."""
    cases = shared("string_in", lambda: _string_cases(oracle))
    for cols, flt, projs, want in cases:
        run(any_ctx, cols, flt, projs, want)
    want = cases[0][3]
    valid = cases[0][0][0].valid
    assert not want[0].data[valid].any() and want[4].data[valid].all() and 0 < want[3].data[valid].sum() < valid.sum()
    assert len(cases[2][3][0]) == int(valid.sum()) and len(cases[3][3][0]) == 0


def _union_case(oracle):
    n = 4001
    rng = np.random.default_rng(61)
    d1 = ["JFK Airport", "JFK Terminal 4", "LaGuardia", "Newark", "Midtown"] + ["zone %02d" % k for k in range(40)]
    d2 = ["Newark", "JFK Cargo", "Harlem", "zone 07", "Bronx"] + ["area %02d" % k for k in range(40)]
    cols = [random_column(rng, B, n, null_frac=0.1), random_column(rng, S, n, null_frac=0.2, dictionary=d1),
            random_column(rng, S, n, null_frac=0.2, dictionary=d2)]
    P, S1, S2 = col("p", 0, B), col("s", 1, S), col("t", 2, S)
    value = fn(Fn.IF, P, S1, S2, t=S)
    many = d1[5:30] + d2[5:30]
    return case(oracle, cols, None, [in_(value, ["Newark", "Harlem", "Midtown", "absent"]), like(value, "JFK%"), in_(value, many),
                                     like(value, "%a %"), value])


def test_string_value_over_a_union_dictionary(any_ctx, oracle):
    """The value is an IF over two dictionaries: membership is decided on the codes of the union the IF produces."""
    cols, flt, projs, want = shared("union", lambda: _union_case(oracle))
    run(any_ctx, cols, flt, projs, want)
    assert 0 < want[1].data.sum() and 0 < want[2].data.sum() < len(want[2])


def _like_cases(oracle):
    n = 4001
    rng = np.random.default_rng(67)
    d = (["JFK Airport", "JFK", "LGA JFK", "Airport", "ports", "100%", "1000", "100% wool", "a_b", "axb", "café", "cafe", "caffè",
          "日本語", "日本", "\U0001F600", "\U0001F600\U0001F600", "", "back\\slash", "line\nbreak"] + ["stop %03d" % k for k in range(200)])
    s = with_validity(Column(S, rng.integers(0, len(d), n, dtype=np.int32), None, d), "random20", rng, [len(d), -1, 2 ** 30])
    s.data[:len(d)] = np.arange(len(d))
    b = Column(I64, np.arange(n, dtype=np.int64))
    S_, B_ = col("s", 0, S), col("b", 1, I64)
    patterns = ["JFK%", "%port", "%or%", "caf_", "100\\%", "100\\%%", "_", "__", "日本%", "a\\_b", "stop 1_7", "stop %", "%\\\\%", "", "%"]
    cols = [s, b]
    return [case(oracle, cols, None, [like(S_, p) for p in patterns[:8]]),
            case(oracle, cols, None, [like(S_, p) for p in patterns[8:]] + [fn(Fn.NOT, like(S_, "stop %"))]),
            case(oracle, cols, like(S_, "stop 0%"), [B_, S_])]


def test_like(any_ctx, oracle):
    """Prefix, suffix, infix, `_` (one code point: an e-acute, a kanji and an emoji each count once), escaped % and _, non-ASCII
    entries, the empty pattern and the empty string."""
    cases = shared("like", lambda: _like_cases(oracle))
    for cols, flt, projs, want in cases:
        run(any_ctx, cols, flt, projs, want)
    first, valid = cases[0][3], cases[0][0][0].valid[:20]
    hits = lambda k: [i for i in range(20) if valid[i] and first[k].data[i]]   # noqa: E731
    assert set(hits(0)) <= {0, 1} and set(hits(3)) <= {10, 11} and set(hits(4)) <= {5} and set(hits(6)) <= {15} and set(hits(7)) <= {14, 16}
    assert len(cases[2][3][0]) > 0


# ---- 5. BOOLEAN -------------------------------------------------------------------------------------------------------
def _boolean_case(oracle):
    n = 4001
    rng = np.random.default_rng(71)
    cols = [random_column(rng, B, n, null_frac=0.2), random_column(rng, I64, n, null_frac=0.1)]
    P, A_ = col("p", 0, B), col("a", 1, I64)
    lt = fn(Fn.CMP_LT, A_, num(0))
    projs = [in_(P, [True]), in_(P, [False]), in_(P, [True, False]), in_(lt, [False, False]), in_(fn(Fn.AND, P, lt), [True])]
    return [case(oracle, cols, None, projs), case(oracle, cols, in_(P, [False]), [A_, P])]


def test_boolean_lists(any_ctx, oracle):
    for cols, flt, projs, want in shared("boolean", lambda: _boolean_case(oracle)):
        run(any_ctx, cols, flt, projs, want)


# ---- 6. positions -----------------------------------------------------------------------------------------------------
def _position_columns():
    n = 20_000
    rng = np.random.default_rng(73)
    d = ["JFK %02d" % k for k in range(30)] + ["LGA %02d" % k for k in range(34)]
    return [Column(I64, rng.integers(0, 1000, n, dtype=np.int64)),
            Column(I64, int_values(rng, n, NARROW, 80, 220), rng.random(n) >= 0.1),
            random_column(rng, S, n, null_frac=0.1, dictionary=d),
            Column(D, rng.integers(-1000, 1000, n).astype(np.float64), rng.random(n) >= 0.2),   # integer valued: sums are exact
            Column(I64, int_values(rng, n, WIDE[:30], -(2 ** 40), 2 ** 40), rng.random(n) >= 0.1)]


def _position_cases(oracle):
    cols = _position_columns()
    K, A_, S_, X, W_ = col("k", 0, I64), col("a", 1, I64), col("s", 2, S), col("x", 3, D), col("w", 4, I64)
    sel = fn(Fn.CMP_LT, K, num(50))                                            # 5 %: the later conjuncts' columns load for live rows only
    return [case(oracle, cols, fn(Fn.AND, fn(Fn.AND, sel, in_(A_, NARROW)), like(S_, "LGA%")), [K, A_, S_]),
            case(oracle, cols, fn(Fn.AND, sel, fn(Fn.NOT, in_(W_, WIDE[:30] + [1, 2, 3]))), [W_, in_(S_, ["JFK 03", "LGA 11", "LGA 12"])]),
            case(oracle, cols, fn(Fn.NOT, fn(Fn.OR, in_(A_, NARROW), like(S_, "JFK 1%"))), [K, fn(Fn.NOT, like(S_, "%2"))])]


def test_positions_in_filters_and_projections(any_ctx, oracle):
    """As a late conjunct behind a selective one, as a projection, under NOT and under OR."""
    for cols, flt, projs, want in shared("positions", lambda: _position_cases(oracle)):
        run(any_ctx, cols, flt, projs, want)
        assert len(want[0]) > 0


def _aggregate_case(oracle):
    cols = _position_columns()
    K, A_, S_, X, W_ = col("k", 0, I64), col("a", 1, I64), col("s", 2, S), col("x", 3, D), col("w", 4, I64)
    flt = fn(Fn.CMP_LT, K, num(900))
    zero = num(0.0)
    exprs = [fn(Fn.IF, in_(A_, NARROW), X, zero), fn(Fn.IF, like(S_, "LGA%"), X, zero), fn(Fn.IF, in_(W_, WIDE[:30] + [1, 2, 3]), X, zero),
             fn(Fn.IF, in_(S_, ["JFK 03", "LGA 11"]), X, zero)]
    aggs = [int(AF.SUM), int(AF.SUM), int(AF.COUNT), int(AF.SUM)]
    keys = [in_(A_, NARROW), like(S_, "JFK%")]
    mode = oracle.BYTECODE_COMPILER
    lowered, lcols = lower([flt] + exprs + keys, cols, oracle, mode)
    lf, le, lk = lowered[0], lowered[1:1 + len(exprs)], lowered[1 + len(exprs):]
    return (cols, flt, keys, exprs, aggs, oracle.filter_aggregate(lcols, lf, le, aggs, mode),
            oracle.filter_groupby(lcols, lf, lk, le, aggs, mode))


def test_inside_if_under_sum_and_as_group_by_key(any_ctx, oracle):
    """SUM(IF(x IN (..), v, 0)) through qe_filter_aggregate; GROUP BY a IN (..), s LIKE '..' through qe_filter_groupby (BOOLEAN
    keys that are NULL where their value is: 3 x 3 groups)."""
    ctx = any_ctx
    cols, flt, keys, exprs, aggs, want_agg, want_gb = shared("aggregate", lambda: _aggregate_case(oracle))
    batch = E.DeviceBatch.from_columns(ctx, cols)
    try:
        cf, ce, ck = ctx.compile(flt), [ctx.compile(e) for e in exprs], [ctx.compile(k) for k in keys]
        vals, nsel = E.filter_aggregate(ctx, batch, cf, ce, aggs)
        assert nsel == want_agg[1] and vals == want_agg[0], (vals, want_agg)
        res = E.filter_groupby(ctx, batch, cf, ck, ce, aggs)
        cs = res.to_columns()
        got = [[c.value(i) for c in cs] for i in range(res.count)]
        res.free()
        assert len(want_gb) == 9
        _rows_equal(got, want_gb, len(keys), aggs, oracle)
    finally:
        batch.free()
