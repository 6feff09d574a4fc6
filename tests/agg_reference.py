"""A plain high-precision reference for SUM / AVG / MIN / MAX / COUNT per group, the error bound the product documents, and
the seeded data sets of the aggregate-numerics tests (test_aggregate_numerics_cpu.py, test_gpu_aggregate_numerics.py).

Pure Python / numpy: no oracle, no GPU.  The reference of a SUM is math.fsum, the correctly rounded EXACT sum -- not a
second rounded summation, which would need twice the bound and would accept twice the error.

The bound.  A sum of c terms evaluated in ANY order and ANY tree shape (sequential, a fixed tree, atomics into an LDS table
merged into a global one, shard partials folded on the host) makes c - 1 rounded additions -- adding into a zero-initialised
accumulator is exact -- and so differs from the exact sum by at most gamma_{c-1} * sum|x|, gamma_k = k*u / (1 - k*u),
u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 4.2).  Additions of doubles cannot
underflow inexactly, so this holds down to the subnormals.  The tests allow gamma_c: the one extra rounding is that of the
reference itself (fsum rounds the exact sum once).  AVG makes one more rounding, the division: gamma_{c+1} * sum|x| / c;
a quotient in the subnormal range is additionally off by up to half the smallest subnormal, 2^-1075 (the standard model
with underflow, ibid. section 2.2) -- a property of the number format that only shows on the `subnormal` data set.
"""
from __future__ import annotations

import math
from fractions import Fraction
from typing import List, Optional, Sequence

import numpy as np

MIN, MAX, SUM, COUNT, AVG = 0, 1, 2, 3, 4          # the reference's AggregationFunction ordinals (ast/Functions.kt:24-26)
FN_NAMES = {MIN: "MIN", MAX: "MAX", SUM: "SUM", COUNT: "COUNT", AVG: "AVG"}
U = 2.0 ** -53
DBL_MAX = 1.7976931348623157e308
DBL_MIN_NORMAL = 2.2250738585072014e-308
_ETA = Fraction(1, 2 ** 1075)                      # half the smallest subnormal: the underflow term of a rounded quotient
NAN_PAYLOAD = float(np.array([0x7ff8000000000123], dtype=np.uint64).view(np.float64)[0])
NAN_NEGATIVE = float(np.array([0xfff8000000000456], dtype=np.uint64).view(np.float64)[0])


def java_min(a: float, b: float) -> float:
    """java.lang.Math.min(double, double): NaN wins, -0.0 is smaller than +0.0."""
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, b) < 0:
        return b
    return a if a <= b else b


def java_max(a: float, b: float) -> float:
    """java.lang.Math.max(double, double): NaN wins, +0.0 is greater than -0.0."""
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, a) < 0:
        return b
    return a if a >= b else b


class Group:
    """One group of the exact reference.  sum / sum_abs are over the FINITE valid values (fsum cannot add infinities);
    the has_* flags say what else the group holds."""
    __slots__ = ("key", "rows", "count", "sum", "sum_abs", "min", "max", "min_abs", "has_nan", "has_pinf", "has_ninf")

    def __repr__(self):
        return (f"Group(key={self.key!r}, rows={self.rows}, count={self.count}, sum={self.sum!r}, sum_abs={self.sum_abs!r}, "
                f"min={self.min!r}, max={self.max!r}, nan={self.has_nan}, +inf={self.has_pinf}, -inf={self.has_ninf})")


def _fold(key, rows: int, vals: Sequence[float]) -> Group:
    g = Group()
    g.key, g.rows, g.count = key, rows, len(vals)
    lo = hi = None
    finite = []
    g.has_nan = g.has_pinf = g.has_ninf = False
    for v in vals:
        if lo is None:
            lo = hi = v                                 # Accumulators.kt:57-80: the first value starts the accumulator
        else:
            lo, hi = java_min(lo, v), java_max(hi, v)
        if v != v:
            g.has_nan = True
        elif v == math.inf:
            g.has_pinf = True
        elif v == -math.inf:
            g.has_ninf = True
        else:
            finite.append(v)
    g.min, g.max = lo, hi
    try:
        g.sum, g.sum_abs = math.fsum(finite), math.fsum(map(abs, finite))
    except OverflowError:                               # sum|x| beyond DBL_MAX: check_aggregate rejects such a group as undecidable
        g.sum, g.sum_abs = math.nan, math.inf
    g.min_abs = min(map(abs, finite)) if finite else None
    return g


def _key_codes(arr, valid):
    """Dense codes of one key column under Double.equals / Object.equals: all NaNs are one key, -0.0 and 0.0 are two,
    NULL is a key of its own."""
    a = np.asarray(arr)
    if a.dtype == np.float64:
        bits = a.view(np.uint64).copy()
        bits[np.isnan(a)] = np.uint64(0x7ff8000000000000)
        a = bits
    uniq, inv = np.unique(a, return_inverse=True)
    inv = inv.astype(np.int64).reshape(-1)
    if valid is not None:
        inv = np.where(np.asarray(valid, dtype=bool), inv, len(uniq))
    return inv, len(uniq) + 1


def exact_groups(key_tuples, valid_keys, values, valid_values=None, selected=None) -> List[Group]:
    """The groups of GroupByAggregation(Filter(Scan)) in order of first appearance among the selected rows.
    key_tuples: one array per key column (n rows each; no key column = one global group, present even when no row is
    selected); valid_keys: one boolean array or None per key column; values: the aggregated DOUBLE input, valid_values its
    validity (None = all valid); selected: the rows the filter keeps (None = all).  A group's key is the tuple of its
    first row's key values (None for NULL)."""
    values = np.asarray(values, dtype=np.float64)
    n = len(values)
    sel = np.ones(n, dtype=bool) if selected is None else np.asarray(selected, dtype=bool)
    vv = np.ones(n, dtype=bool) if valid_values is None else np.asarray(valid_values, dtype=bool)
    valid_keys = list(valid_keys) if valid_keys is not None else [None] * len(key_tuples)
    rows = np.nonzero(sel)[0]
    if not key_tuples:
        return [_fold((), len(rows), values[rows][vv[rows]].tolist())]
    comb = np.zeros(n, dtype=np.int64)
    for arr, valid in zip(key_tuples, valid_keys):
        inv, k = _key_codes(arr, valid)
        _, comb = np.unique(comb * k + inv, return_inverse=True)
        comb = comb.astype(np.int64).reshape(-1)
    uniq, first, inv = np.unique(comb[rows], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # groups by first appearance
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    gid = rank[inv.reshape(-1)]
    by_group = np.argsort(gid, kind="stable")                # rows of a group stay in row order
    srows = rows[by_group]
    bounds = np.searchsorted(gid[by_group], np.arange(len(uniq) + 1))
    svals, svalid = values[srows].tolist(), vv[srows].tolist()
    out = []
    for g in range(len(uniq)):
        b, e = int(bounds[g]), int(bounds[g + 1])
        r0 = int(srows[b])
        key = tuple(None if (v is not None and not v[r0]) else np.asarray(a)[r0].item() for a, v in zip(key_tuples, valid_keys))
        out.append(_fold(key, e - b, [x for x, ok in zip(svals[b:e], svalid[b:e]) if ok]))
    return out


def _gamma(k: int) -> Fraction:
    ku = Fraction(k, 2 ** 53)
    return ku / (1 - ku)


def sum_bound(count: int, sum_abs: float) -> float:
    """gamma_c * sum|x|: how far a SUM of `count` doubles, added in any order, may be from the exact sum."""
    return float(_gamma(count) * Fraction(sum_abs)) if count > 0 else 0.0


def avg_bound(count: int, sum_abs: float) -> float:
    """gamma_{c+1} * sum|x| / c: the SUM's bound and the rounding of the division."""
    return float(_gamma(count + 1) * Fraction(sum_abs) / count) if count > 0 else 0.0


def _bits(x: float) -> int:
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def _same(got: float, want: float) -> bool:
    """Bit pattern equality (+0.0 != -0.0); any NaN equals any NaN (helpers.assert_columns_equal)."""
    return (got != got and want != want) or _bits(got) == _bits(want)


def decided_sum(group: Group):
    """What SUM must be when the input decides it: ("nan" | "+inf" | "-inf" | "finite").  Raises on a group whose finite
    values could overflow in one order of additions and not in another: such an input is an error of the test."""
    if group.has_nan:
        return "nan"
    if not group.sum_abs < DBL_MAX / 2:
        raise ValueError(f"undecidable input: sum|x| = {group.sum_abs!r} of group {group.key!r} can overflow in some order")
    if group.has_pinf and group.has_ninf:
        return "nan"
    if group.has_pinf:
        return "+inf"
    if group.has_ninf:
        return "-inf"
    return "finite"


def check_aggregate(fn: int, got: Optional[float], group: Group, what: str = "") -> float:
    """Assert that `got` is an acceptable value of aggregate `fn` over `group`.  Returns |got - exact| / bound for a
    finite SUM / AVG (0.0 where the comparison is exact), so that callers can report how much of the bound was used; an AVG
    in the subnormal range reports 0.0: there the rounding of the quotient alone may use the whole bound."""
    fn = int(fn)

    def require(ok: bool, want: str) -> None:
        if not ok:
            raise AssertionError(f"{what}: {FN_NAMES[fn]} of {group!r}: got {got!r}, want {want}")

    if fn == COUNT:
        require(got is not None and got == group.count, "the count")
        return 0.0
    if group.count == 0:
        require(got is None, "NULL (no valid value)")
        return 0.0
    require(got is not None, "a value")
    got = float(got)
    if fn in (MIN, MAX):
        want = group.min if fn == MIN else group.max
        require(_same(got, want), repr(want))
        return 0.0
    kind = decided_sum(group)
    if kind == "nan":
        require(got != got, "NaN")
        return 0.0
    if kind != "finite":
        require(got == (math.inf if kind == "+inf" else -math.inf), kind)
        return 0.0
    c = group.count
    if group.sum_abs == 0.0:                   # only zeros: the accumulator starts from +0.0 (Accumulators.kt:40), -0.0 never comes out
        require(_same(got, 0.0), "+0.0")
        return 0.0
    require(math.isfinite(got), f"{group.sum!r} (exact sum)")
    # the common case without big rationals, in doubles: the difference is rounded once (relative u), SUM's reference is the
    # exact sum rounded by fsum (covered by gamma_c, see the module docstring), AVG's reference adds the rounding of its quotient
    ref = group.sum if fn == SUM else group.sum / c
    if got == ref and (fn == SUM or c == 1):
        return 0.0
    k = c * U if fn == SUM else (c + 1) * U
    quick, room = abs(got - ref), k / (1.0 - k) * (group.sum_abs if fn == SUM else group.sum_abs / c)      # (the bound, in doubles)
    if quick + (0.0 if fn == SUM else U * abs(ref)) <= room * (1.0 - 1e-12) and abs(ref) >= DBL_MIN_NORMAL:
        return quick / room
    # otherwise the comparison itself is made in exact arithmetic: no rounding of ours eats into the bound
    if fn == SUM:
        exact, bound = Fraction(group.sum), _gamma(c) * Fraction(group.sum_abs)
    else:
        exact, bound = Fraction(group.sum) / c, _gamma(c + 1) * Fraction(group.sum_abs) / c + _ETA
    err = abs(Fraction(got) - exact)
    require(err <= bound, f"{float(exact)!r} (exact): |error| {float(err):.3e} > bound {float(bound):.3e}")
    return float(err / bound) if fn == SUM or abs(exact) >= DBL_MIN_NORMAL else 0.0


# ---- the data sets ---------------------------------------------------------------------------------------------------
DATASETS = ("same_magnitude", "wide_range", "cancelling", "specials", "subnormal")
FILTER_LIMIT = 500           # the filter of every case is y < 500 with y uniform in [-1000, 1000): keeps 75 % of the rows
SPECIAL_GROUPS = 16          # `specials` plants its cases in group ids 0 .. 15


class Data:
    """gid: the group id of every row (routes turn it into their key columns); x: the DOUBLE value column and its validity;
    y: INT64, never NULL -- the filter's column and the second operand of x + y."""

    def __init__(self, name, gid, ngroups, x, x_valid, y):
        self.name, self.gid, self.ngroups, self.x, self.x_valid, self.y = name, gid, ngroups, x, x_valid, y
        self.n = len(gid)

    @property
    def selected(self):
        return self.y < FILTER_LIMIT

    def inputs(self):
        """The aggregated expressions, evaluated in numpy with every operation rounded on its own (the product is built
        with -ffp-contract=off): x, x * 0.1, x + y."""
        with np.errstate(all="ignore"):
            return {"x": self.x, "x*0.1": self.x * 0.1, "x+y": self.x + self.y.astype(np.float64)}


def make_gid(rng: np.random.Generator, n: int, ngroups: int, skewed: bool = False) -> np.ndarray:
    gid = rng.integers(0, ngroups, n).astype(np.int64)
    if skewed:                                             # 90 % of the rows in one group
        gid[rng.random(n) < 0.9] = ngroups // 2
    return gid


def make_data(name: str, n: int, ngroups: int, seed: int = 1, skewed: bool = False) -> Data:
    rng = np.random.default_rng([seed, n, ngroups, DATASETS.index(name)])
    gid = make_gid(rng, n, ngroups, skewed)
    y = rng.integers(-1000, 1000, n).astype(np.int64)
    valid = rng.random(n) > 0.2
    if name == "same_magnitude":
        x = rng.uniform(1.0, 2.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    elif name == "wide_range":
        x = rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 9, n)
    elif name == "cancelling":
        # rows in pairs (+v, -v) of one group, the partners scattered across the batch, both on the same side of the filter
        # and both valid; every 64th pair is a small residue instead
        perm = rng.permutation(n)
        half = n // 2
        a, b = perm[:half], perm[half:2 * half]
        v = rng.uniform(1e15, 2e15, half)
        x = rng.normal(0, 1, n)                            # the odd row out (if any) is a residue
        x[a], x[b] = v, -v
        residue = rng.random(half) < 1 / 64
        x[a[residue]] = rng.normal(0, 1, int(residue.sum()))
        x[b[residue]] = rng.normal(0, 1, int(residue.sum()))
        gid[b], y[b], valid[b] = gid[a], y[a], valid[a]
    elif name == "subnormal":
        x = rng.integers(-1000, 1001, n).astype(np.float64) * 5e-324
    elif name == "specials":
        x = rng.normal(0, 100, n)
        zeros = rng.random(n) < 0.02
        x[zeros] = np.where(rng.random(int(zeros.sum())) < 0.5, 0.0, -0.0)
        _plant_specials(rng, gid, x, valid, y)
    else:
        raise ValueError(name)
    return Data(name, gid, ngroups, x, valid, y)


def _plant_specials(rng, gid, x, valid, y) -> None:
    """Group ids 0 .. 15 get the compositions listed in SPECIAL_CASES (a group that has no row in a small batch simply
    does not exist)."""
    def rows(g, selected_only=True):
        r = np.nonzero(gid == g)[0]
        return r[y[r] < FILTER_LIMIT] if selected_only else r

    def put(g, where, value):
        r = rows(g)
        if len(r):
            i = r[{"first": 0, "last": -1, "middle": len(r) // 2}[where]]
            x[i], valid[i] = value, True

    x[gid == 0] = -0.0                                               # only -0.0
    r = rows(1, False)
    x[r] = np.where(np.arange(len(r)) % 3 == 0, 0.0, -0.0)           # -0.0 and +0.0
    valid[r[:2]] = True
    put(2, "middle", math.nan)                                       # one NaN among many
    put(3, "first", NAN_PAYLOAD)                                     # NaN first
    put(4, "last", NAN_NEGATIVE)                                     # NaN last (sign bit set)
    put(5, "middle", math.inf)                                       # +Inf only
    put(6, "first", math.inf)                                        # both infinities
    put(6, "last", -math.inf)
    valid[gid == 7] = False                                          # every value NULL
    r = rows(8)
    valid[gid == 8] = False                                          # exactly one valid value (among the selected rows)
    if len(r):
        valid[r[len(r) // 3]] = True
    r = rows(9, False)                                               # a NaN that the filter removes
    r = r[y[r] >= FILTER_LIMIT]
    if len(r):
        x[r[0]], valid[r[0]] = math.nan, True
    put(10, "first", 5e-324)                                         # the smallest subnormals among ordinary values
    put(10, "last", -5e-324)
    put(11, "middle", DBL_MAX / 4)                                   # huge, one per group: sum|x| stays below DBL_MAX / 2
    put(12, "middle", -DBL_MAX / 4)
    put(13, "last", -math.inf)                                       # -Inf only
    r = rows(14)                                                     # only subnormals: +-5e-324
    x[gid == 14] = 5e-324
    x[r[::2]] = -5e-324
    put(15, "first", -0.0)                                           # -0.0 first, then ordinary values


# ---- the batches of the GPU suite: route -> (kind of key, distinct keys, rows (a ragged size)) ---------------------------------
ROUTE_SHAPES = {
    "dense_lds_table":                 ("dict_bool", 74, 200_003),       # 37 dictionary keys x boolean: LDS-privatised table
    "dense_partitioned_3000":          ("dict", 3000, 300_017),          # table beyond LDS: count -> scan -> scatter -> qe_gb_aggregate
    "dense_partitioned_300000":        ("dict", 300_000, 400_003),       # ... with several partition slices and their merge
    "dense_global_atomics":            ("dict", 3000, 300_017),
    "hashed_lds_tables":               ("double", 24, 200_003),          # few DOUBLE keys: they stay in the workgroups' LDS hash tables
    "hashed_dense_ids_double":         ("double", 5000, 200_003),        # keys resolved to dense ids, then the dense kernels
    "hashed_dense_ids_int64":          ("int64", 150_000, 600_011),
    "hashed_global_atomics":           ("int64", 150_000, 600_011),
    "hash_partitioned_lines":          ("double", 2000, 250_003),        # < 4096 groups: finished on the host
    "hash_partitioned_header_records": ("double", 2000, 250_003),
    "hash_partitioned_device_finish":  ("double", 5000, 250_003),        # >= 4096 groups: finished on the device
    "hash_partitioned_device_small":   ("double", 74, 250_003),
}
SKEWED_ROUTES = ("dense_lds_table", "dense_partitioned_3000", "hashed_lds_tables", "hashed_dense_ids_double")
PARTITIONED_SIZES = (1, 63, 4096, 4097, 65_536, 65_537, 131_077)        # tiles of 4096 rows, chunks of 16 tiles
SIZES_ROUTE, SIZES_DATASETS = "dense_partitioned_3000", ("same_magnitude", "wide_range")
GLOBAL_SHAPE = (74, 300_017)                                            # the global aggregate's batches (group ids unused)


# ---- a data set as the columns, keys and aggregates of one plan -------------------------------------------------------
AGG_INPUTS = ("x", "x", "x", "x", "x", "x*0.1", "x+y")
AGG_FNS = (SUM, AVG, MIN, MAX, COUNT, SUM, AVG)
KEY_KINDS = ("dict_bool", "dict", "double", "int64", "none")


class Case:
    """One data set behind one kind of group key: `cols` = key columns, x, y; `keys` / `exprs` / `aggs` / `flt` as the engine and
    the oracle take them; key_arrays / key_valids as exact_groups takes them; result_key(group) = the key values a result
    row of that group must show."""

    def __init__(self, kind: str, data: Data):
        from queryengine_amd import (Column, ColumnExpression, DataType, Function, FunctionExpression,
                                     NumericLiteralExpression)
        D, I64, B, S = DataType.DOUBLE, DataType.INT64, DataType.BOOLEAN, DataType.STRING
        self.kind, self.data = kind, data
        gid, ng = data.gid, data.ngroups
        self.dictionary = None
        if kind == "dict_bool":                  # ng = 2 * (dictionary entries); one NULL string key, one NULL boolean key
            nd = ng // 2
            self.dictionary = ["k%03d" % i for i in range(nd)]
            code, p = (gid % nd).astype(np.int32), (gid // nd) % 2 == 1
            sv, pv = gid != ng - 1, gid != ng - 2
            kcols, ktypes = [Column(S, code, sv, self.dictionary), Column(B, p, pv)], [S, B]
            self.key_arrays, self.key_valids = [code, p], [sv, pv]
        elif kind == "dict":
            self.dictionary = ["k%06d" % i for i in range(ng)]
            code, sv = gid.astype(np.int32), gid != ng - 1
            kcols, ktypes = [Column(S, code, sv, self.dictionary)], [S]
            self.key_arrays, self.key_valids = [code], [sv]
        elif kind == "double":                   # Double.equals keys: NaN, -0.0, 0.0, +-Inf are keys like any other; one NULL key
            pool = np.random.default_rng(7).normal(0, 1e6, ng)
            special = [math.nan, -0.0, 0.0, math.inf, -math.inf]
            pool[ng - 1 - len(special):ng - 1] = special
            assert len(np.unique(pool[~np.isnan(pool)])) >= ng - 2          # (-0.0 == 0.0 for np.unique)
            k, kv = pool[gid], gid != ng - 1
            kcols, ktypes = [Column(D, k, kv)], [D]
            self.key_arrays, self.key_valids = [k], [kv]
        elif kind == "int64":
            pool = np.unique(np.random.default_rng(7).integers(-2 ** 62, 2 ** 62, 2 * ng))[:ng]
            pool = np.random.default_rng(8).permutation(pool)
            assert len(pool) == ng
            k, kv = pool[gid], gid != ng - 1
            kcols, ktypes = [Column(I64, k, kv)], [I64]
            self.key_arrays, self.key_valids = [k], [kv]
        elif kind == "none":
            kcols, ktypes = [], []
            self.key_arrays, self.key_valids = [], []
        else:
            raise ValueError(kind)
        nk = len(kcols)
        self.cols = kcols + [Column(D, data.x, data.x_valid), Column(I64, data.y)]
        self.keys = [ColumnExpression("k%d" % i, i, t) for i, t in enumerate(ktypes)]
        X, Y = ColumnExpression("x", nk, D), ColumnExpression("y", nk + 1, I64)
        by_name = {"x": X, "x*0.1": FunctionExpression(Function.MUL, [X, NumericLiteralExpression(0.1)], D),
                   "x+y": FunctionExpression(Function.ADD, [X, Y], D)}
        self.exprs = [by_name[name] for name in AGG_INPUTS]
        self.aggs = list(AGG_FNS)
        self.flt = FunctionExpression(Function.CMP_LT, [Y, NumericLiteralExpression(float(FILTER_LIMIT))], B)
        self._exact = {}

    def result_key(self, group: Group):
        if self.kind in ("dict_bool", "dict"):
            return [None if group.key[0] is None else self.dictionary[group.key[0]]] + [None if k is None else bool(k) for k in group.key[1:]]
        return list(group.key)

    def exact(self, filtered: bool):
        """{input name: [Group, ...]} of the exact reference, with or without the filter (computed once)."""
        if filtered not in self._exact:
            sel = self.data.selected if filtered else None
            self._exact[filtered] = {name: exact_groups(self.key_arrays, self.key_valids, v, self.data.x_valid, sel)
                                     for name, v in self.data.inputs().items()}
        return self._exact[filtered]


def keys_equal(got, want) -> bool:
    """Key values of a result row against the reference's: Double.equals for doubles (NaN == NaN, -0.0 != 0.0)."""
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        if isinstance(b, float):
            if a is None or not _same(float(a), b):
                return False
        elif a != b or (a is None) != (b is None):
            return False
    return True


def check_rows(case: Case, filtered: bool, rows, what: str, checked=None) -> float:
    """rows = [[key values..., aggregate values...], ...] of a group-by over `case`: same groups in the same (first appearance)
    order as the exact reference, every aggregate within check_aggregate.  Returns the largest |error| / bound seen.  `checked`: the rows of an earlier
    execution that passed this check -- a row that repeats its values bit for bit is not judged a second time."""
    exact = case.exact(filtered)
    ref = exact["x"]
    assert len(rows) == len(ref), f"{what}: {len(rows)} groups, the exact reference has {len(ref)}"
    nk, worst = len(case.keys), 0.0
    per_input = [exact[name] for name in AGG_INPUTS]
    for i, row in enumerate(rows):
        # (list equality is float equality: a NaN never repeats, and -0.0 == 0.0, so a row that holds a zero is always judged again)
        if checked is not None and len(checked) == len(rows) and row == checked[i] and 0.0 not in row[nk:]:
            continue
        want = case.result_key(ref[i])
        assert keys_equal(row[:nk], want), f"{what}: group {i} has key {row[:nk]!r}, the exact reference {want!r}"
        for j, fn in enumerate(AGG_FNS):
            try:
                r = check_aggregate(fn, row[nk + j], per_input[j][i])
            except AssertionError as e:
                raise AssertionError(f"{what}, group {i} key {want!r}, {FN_NAMES[fn]}({AGG_INPUTS[j]}){e}") from None
            if r > worst:
                worst = r
    return worst
