"""SUM / AVG / MIN / MAX / COUNT on fractional and special VALUES through every accumulation route of the group-by and
through the global aggregate, against the exact reference of agg_reference.py (math.fsum, Java Math.min/max) within the
documented bound gamma_c * sum|x| -- no other tolerance.  test_aggregate_numerics_cpu.py proves on the CPU that the bound
sees a lost, a doubled and a misrouted row and that no data set holds an undecidable group.

One schema and one expression list per route: the data sets differ in data, not in plan, so a plan is compiled once.
Every test asserts through ctx.last_form and the group count that the intended route ran.  Each test prints the largest
|got - exact| / bound it saw (`pytest -s` shows it)."""
import re

import numpy as np
import pytest

import agg_reference as R
from queryengine_amd import native as N

pytestmark = pytest.mark.gpu

DENSE, HASHED, HASH_PARTITIONED = N.FORM_GROUPBY_DENSE, N.FORM_GROUPBY_HASHED, N.FORM_GROUPBY_HASH_PARTITIONED
GLOBAL_ATOMICS_DENSE, GLOBAL_ATOMICS_HASHED = 256, 131072                    # debug bits of tuning[5]
FORCE_HP, HP_HEADER_RECORDS, FINISH_ON_DEVICE = 8388608, 33554432, 67108864
SCATTER_CLOCKS = 64                                                          # a diagnostic BUILD of the partitioned passes

# route -> (tuning[5], the form that must run, executions per plan, fewest groups, most groups); its key kind, key count and
# rows are agg_reference.ROUTE_SHAPES[route].  ctx.last_form tells the three forms apart, not the routes inside a form: those
# are chosen by state that STICKS to a plan (one per context, schema, filter, keys and aggregates) from one execution to the
# next -- use_ids (set once an execution met more than 64 keys or keys that do not fit the LDS tables: every later execution
# builds dense ids), ids_overflow, id_capacity / hash_capacity, and for the hash-partitioned form known_keys (sizes the
# partitions) and hp_failed.  So every route has a context, and with it plans, of its own (`contexts` below): what one route
# leaves behind cannot steer another, whatever the order or selection of the tests.  Inside a route every data set has the
# same number of keys, and the group bounds below state what keeps it on its route: at most 64 keys never set use_ids
# (hashed_lds_tables), more always do on the first execution (the dense-id routes); the hash-partitioned result is finished
# on the host below 4096 groups and on the device from there on (or always, debug bit 67108864).
ROUTES = {
    "dense_lds_table":                 (0, DENSE, 2, 74, 74),
    "dense_partitioned_3000":          (0, DENSE, 2, 2900, 3000),
    "dense_partitioned_300000":        (0, DENSE, 2, 100_000, 300_000),
    "dense_global_atomics":            (GLOBAL_ATOMICS_DENSE, DENSE, 2, 2900, 3000),
    "hashed_lds_tables":               (0, HASHED, 2, 24, 24),
    "hashed_dense_ids_double":         (0, HASHED, 2, 1000, 5000),
    "hashed_dense_ids_int64":          (0, HASHED, 2, 100_000, 150_000),
    "hashed_global_atomics":           (GLOBAL_ATOMICS_HASHED, HASHED, 2, 100_000, 150_000),
    "hash_partitioned_lines":          (FORCE_HP, HASH_PARTITIONED, 3, 1900, 2000),
    "hash_partitioned_header_records": (FORCE_HP | HP_HEADER_RECORDS, HASH_PARTITIONED, 3, 1900, 2000),
    "hash_partitioned_device_finish":  (FORCE_HP, HASH_PARTITIONED, 3, 4096, 5000),
    "hash_partitioned_device_small":   (FORCE_HP | FINISH_ON_DEVICE, HASH_PARTITIONED, 3, 74, 74),
}
assert set(ROUTES) == set(R.ROUTE_SHAPES)
IDS_FROM, DEVICE_FINISH_FROM = 64, 4096
assert ROUTES["hashed_lds_tables"][4] <= IDS_FROM < ROUTES["hashed_dense_ids_double"][3]
assert ROUTES["hash_partitioned_lines"][4] < DEVICE_FINISH_FROM <= ROUTES["hash_partitioned_device_finish"][3]


@pytest.fixture(scope="module")
def contexts(native_lib):
    """One context per ROUTE (and one each for the global aggregate and query()) for the whole module: a route's plans are
    compiled once and no other route touches their state."""
    from queryengine_amd import engine as E
    made = {}

    def get(route: str, word=None):
        if route not in made:
            if word is None:
                word = ROUTES[route][0] if route in ROUTES else 0
            made[route] = E.Context(device=0, tuning=[0, 0, 0, 0, 0, word, 0, 0] if word else [])
        return made[route]
    yield get
    for ctx in made.values():
        ctx.close()


def _rows(res):
    """Result -> [[key values..., aggregate values...], ...] (None = NULL), and the raw columns."""
    cols = res.to_columns()
    lists = []
    for c in cols:
        vals = c.data.tolist()
        if c.dictionary is not None:
            vals = [c.dictionary[v] for v in vals]
        if c.valid is not None:
            vals = [v if ok else None for v, ok in zip(vals, c.valid.tolist())]
        lists.append(vals)
    return [list(r) for r in zip(*lists)], cols


def _assert_exact_columns_repeat(case, first, second, what):
    """COUNT / MIN / MAX of two executions: bit-identical, NULLs included (SUM / AVG come from atomics: identity is not promised)."""
    nk = len(case.keys)
    for j, fn in enumerate(R.AGG_FNS):
        if fn in (R.COUNT, R.MIN, R.MAX):
            a, b = first[nk + j], second[nk + j]
            av = a.valid if a.valid is not None else np.ones(len(a), bool)
            bv = b.valid if b.valid is not None else np.ones(len(b), bool)
            assert np.array_equal(av, bv) and np.array_equal(a.data[av].view(np.uint64), b.data[bv].view(np.uint64)), \
                f"{what}: {R.FN_NAMES[fn]}({R.AGG_INPUTS[j]}) differs between two executions"


def _run_groupby(contexts, route, name, n=None, skewed=False):
    from queryengine_amd import engine as E
    (kind, ngroups, rows), (word, form, reps, fewest, most) = R.ROUTE_SHAPES[route], ROUTES[route]
    fewest, n = (fewest, rows) if n is None else (1, n)        # (a smaller batch of the size sweep holds fewer groups)
    ctx = contexts(route)
    case = R.Case(kind, R.make_data(name, n, ngroups, skewed=skewed))
    batch = E.DeviceBatch.from_columns(ctx, case.cols)
    keys, exprs = [ctx.compile(k) for k in case.keys], [ctx.compile(e) for e in case.exprs]
    worst = 0.0
    try:
        for filtered in (False, True):
            cf = ctx.compile(case.flt) if filtered else None
            what = f"route {route}, data set {name}{' (skewed)' if skewed else ''}, {n} rows, filter {filtered}"
            first = first_rows = None
            for rep in range(reps):
                res = E.filter_groupby(ctx, batch, cf, keys, exprs, case.aggs)
                got, cols = _rows(res)
                res.free()
                assert ctx.last_form == form, f"{what}, execution {rep}: ran form {ctx.last_form}, not {form}"
                worst = max(worst, R.check_rows(case, filtered, got, f"{what}, execution {rep}", first_rows))
                if first is None:
                    first, first_rows = cols, got
                else:
                    _assert_exact_columns_repeat(case, first, cols, what)
            ng = len(case.exact(filtered)["x"])
            assert fewest <= ng <= most, f"{what}: {ng} groups, the route needs {fewest} .. {most}"
            if name == "subnormal":
                # integer multiples of 2^-1074: every order of additions gives the exact sum, so SUM(x) is asserted bit for bit
                nk = len(case.keys)
                for i, (row, g) in enumerate(zip(got, case.exact(filtered)["x"])):
                    if g.count:
                        assert row[nk] == g.sum and np.signbit(row[nk]) == np.signbit(g.sum), \
                            f"{what}: group {i} key {row[:nk]!r} count {g.count}: SUM {row[nk]!r}, exact {g.sum!r} (a flushed subnormal?)"
    finally:
        batch.free()
    print(f"NUMERICS route={route} data={name}{'/skewed' if skewed else ''} rows={n} worst_error_over_bound={worst:.3g}")
    return case


@pytest.mark.parametrize("name", R.DATASETS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_group_by_route_is_within_the_bound_of_the_exact_sum(contexts, route, name):
    """Every data set through every accumulation route, with and without the filter, two executions (three of the
    hash-partitioned form): the exact reference's groups in its order, COUNT / MIN / MAX exact and identical between
    executions, SUM / AVG within gamma_c * sum|x| of the exact sum, NaN / +-Inf / -0.0 / all-NULL groups as decided."""
    _run_groupby(contexts, route, name)


@pytest.mark.parametrize("name", ["same_magnitude", "wide_range"])
@pytest.mark.parametrize("route", R.SKEWED_ROUTES)
def test_group_by_with_one_group_holding_most_rows(contexts, route, name):
    """90 % of the rows in one group: its table entry takes most atomics and its bound is the widest -- it still sees a
    single lost row (every |x| of `same_magnitude` is more than twice that bound)."""
    case = _run_groupby(contexts, route, name, skewed=True)
    groups = case.exact(True)["x"]
    big = max(groups, key=lambda g: g.count)
    assert big.count > 0.5 * case.data.n
    if name == "same_magnitude":
        assert big.min_abs > 2 * R.sum_bound(big.count, big.sum_abs)


@pytest.mark.parametrize("name", R.SIZES_DATASETS)
@pytest.mark.parametrize("n", R.PARTITIONED_SIZES)
def test_group_by_partitioned_sizes_are_within_the_bound(contexts, n, name):
    """The partitioned passes around their tile (4096 rows) and chunk (16 tiles) edges, on fractional values."""
    _run_groupby(contexts, R.SIZES_ROUTE, name, n=n)


# One row past a chunk edge of the partitioned passes, on the key-range form and on the forced hash-partitioned form; each test
# has contexts of its own (a debug word of its own is a build of its own).
PASSES_ROUTES, PASSES_ROWS = ("dense_partitioned_3000", "hash_partitioned_lines"), 65_537


def _passes_case(contexts, route, purpose, extra_word=0):
    from queryengine_amd import engine as E
    (kind, ngroups, _), (word, form, _, _, _) = R.ROUTE_SHAPES[route], ROUTES[route]
    ctx = contexts(f"{route}/{purpose}", word | extra_word)
    case = R.Case(kind, R.make_data("same_magnitude", PASSES_ROWS, ngroups))
    batch = E.DeviceBatch.from_columns(ctx, case.cols)
    keys, exprs = [ctx.compile(k) for k in case.keys], [ctx.compile(e) for e in case.exprs]

    def execute(flt):
        res = E.filter_groupby(ctx, batch, ctx.compile(flt) if flt is not None else None, keys, exprs, case.aggs)
        got, _ = _rows(res)
        res.free()
        assert ctx.last_form == form, f"route {route}: ran form {ctx.last_form}, not {form}"
        return got
    return case, batch, form, execute


@pytest.mark.parametrize("route", PASSES_ROUTES)
def test_group_by_partitioned_passes_when_the_filter_keeps_no_row(contexts, route):
    """No record to scatter: 0 groups from the intended form, and the next execution on the same context -- every row kept --
    is still correct (the passes leave their profile bracket closed and the control words usable), twice over."""
    from queryengine_amd import FunctionExpression, Function, NumericLiteralExpression, DataType, ColumnExpression
    case, batch, _, execute = _passes_case(contexts, route, "nothing_kept")
    y = ColumnExpression("y", len(case.keys) + 1, DataType.INT64)
    nothing = FunctionExpression(Function.CMP_LT, [y, NumericLiteralExpression(-5000.0)], DataType.BOOLEAN)
    try:
        for rep in range(2):
            assert execute(nothing) == [], f"route {route}, execution {rep}: groups from a filter that keeps no row"
            R.check_rows(case, False, execute(None), f"route {route}, {PASSES_ROWS} rows, after an empty selection, execution {rep}")
    finally:
        batch.free()


@pytest.mark.parametrize("route", PASSES_ROUTES)
def test_group_by_scatter_clocks_diagnostic_prints_one_line_per_scatter(contexts, route, capfd):
    """tuning[5] bit 64: the diagnostic build of the scatter pass.  The rows are those of the exact reference, and stderr holds
    exactly one `qe_gb_scatter` phases line per execution (each scatters records), labelled on the hash-partitioned form."""
    case, batch, form, execute = _passes_case(contexts, route, "scatter_clocks", SCATTER_CLOCKS)
    try:
        for filtered in (False, True):
            capfd.readouterr()
            got = execute(case.flt if filtered else None)
            err = capfd.readouterr().err
            R.check_rows(case, filtered, got, f"route {route}, scatter clocks, {PASSES_ROWS} rows, filter {filtered}")
            lines = [line for line in err.splitlines() if line.startswith("qe_gb_scatter")]
            assert len(lines) == 1, f"route {route}, filter {filtered}: {len(lines)} phases lines in {err!r}"
            assert re.search(r" phases, clocks per wave \(grid \d+ x \d+ waves\): issue loads \d+ \| flush \(stores\) \d+ \| LDS sort \d+ \| "
                             r"wait loads \+ evaluate \d+ \| chunk drain \d+$", lines[0]), lines[0]
            assert lines[0].startswith("qe_gb_scatter (hash-partitioned) phases") == (form == HASH_PARTITIONED), lines[0]
            assert lines[0].startswith("qe_gb_scatter phases") == (form == DENSE), lines[0]
    finally:
        batch.free()


@pytest.mark.parametrize("name", R.DATASETS)
def test_global_aggregate_is_deterministic_and_within_the_bound(contexts, name):
    """qe_filter_aggregate: no keys; without a filter, with one, with an empty selection.  The fixed-shape tree is
    documented as deterministic: three executions on one context and one on a fresh context give bit-identical SUM / AVG
    (and everything else), within the bound of the exact sum."""
    from queryengine_amd import FunctionExpression, Function, NumericLiteralExpression, DataType, ColumnExpression
    from queryengine_amd import engine as E
    case = R.Case("none", R.make_data(name, R.GLOBAL_SHAPE[1], R.GLOBAL_SHAPE[0]))
    nothing = FunctionExpression(Function.CMP_LT, [ColumnExpression("y", 1, DataType.INT64), NumericLiteralExpression(-5000.0)], DataType.BOOLEAN)
    fresh = E.Context(device=0)
    worst = 0.0
    try:
        for filtered, flt in ((False, None), (True, case.flt), (None, nothing)):
            what = f"route global aggregate, data set {name}, filter {filtered}"
            runs = []
            for ctx in (contexts("global"), contexts("global"), contexts("global"), fresh):
                batch = E.DeviceBatch.from_columns(ctx, case.cols)
                vals, nsel = E.filter_aggregate(ctx, batch, ctx.compile(flt) if flt is not None else None,
                                                [ctx.compile(e) for e in case.exprs], case.aggs)
                batch.free()
                runs.append(vals)
                if filtered is None:
                    assert nsel == 0 and vals == [None, None, None, None, 0.0, None, None], f"{what}: {vals}"
                else:
                    assert nsel == case.exact(filtered)["x"][0].rows
                    worst = max(worst, R.check_rows(case, filtered, [vals], what))
            for other in runs[1:]:
                for a, b, fn, inp in zip(runs[0], other, R.AGG_FNS, R.AGG_INPUTS):
                    assert (a is None and b is None) or R._same(a, b), f"{what}: {R.FN_NAMES[fn]}({inp}) {a!r} then {b!r}: not deterministic"
    finally:
        fresh.close()
    print(f"NUMERICS route=global_aggregate data={name} rows={case.data.n} worst_error_over_bound={worst:.3g}")


def test_query_end_to_end_on_special_values(contexts):
    """SELECT k, SUM(x), AVG(x), MIN(x), MAX(x), COUNT(x) FROM t WHERE y < 500 on the `specials` data set through query():
    the finishing projection and Column.value see NaN, +-Inf, -0.0 and NULL aggregates too."""
    from queryengine_amd import ColumnarTable, DataType, Field, Schema, TableRegistry
    from queryengine_amd.planner import Mode, query
    case = R.Case("dict", R.make_data("specials", 200_003, 24))
    t = ColumnarTable(Schema([Field("k", DataType.STRING), Field("x", DataType.DOUBLE), Field("y", DataType.INT64)]), case.cols)
    reg = TableRegistry()
    reg.register("t", t)
    rows = query(reg, f"SELECT k, SUM(x), AVG(x), MIN(x), MAX(x), COUNT(x) FROM t WHERE y < {R.FILTER_LIMIT}", Mode.GPU_FUSED, ctx=contexts("query"))
    groups = case.exact(True)["x"]
    assert len(rows) == len(groups) == 24
    for row, g in zip(rows, groups):
        want = case.result_key(g)
        assert R.keys_equal(row[:1], want), (row, want)
        for got, fn in zip(row[1:], (R.SUM, R.AVG, R.MIN, R.MAX, R.COUNT)):
            R.check_aggregate(fn, got, g, f"query(), group {want!r}")
        assert isinstance(row[5], int)                                     # COUNT keeps the reference's Int
    by_key = {r[0]: r for r in rows}
    assert by_key["k000007"][1:] == [None, None, None, None, 0]            # every value NULL
    z = by_key["k000000"]                                                  # only -0.0: SUM and AVG +0.0, MIN and MAX -0.0
    assert [float(v) for v in z[1:5]] == [0.0] * 4 and [bool(np.signbit(v)) for v in z[1:5]] == [False, False, True, True]
    assert all(v != v for v in by_key["k000002"][1:5]) and by_key["k000006"][3:5] == [float("-inf"), float("inf")]
