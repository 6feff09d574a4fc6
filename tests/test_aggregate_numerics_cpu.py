"""The exact reference, the error bound and the data sets of the aggregate-numerics suite, proven on the CPU before a GPU
sees them (the GPU half is test_gpu_aggregate_numerics.py): the sequential oracle stays within the bound on every data
set, the bound is tight enough to see one lost / doubled / misrouted row, and the sharded merge of per-shard partials
passes the same check."""
import math

import numpy as np
import pytest

import agg_reference as R
from queryengine_amd import distributed as Dist

N_ROWS = 200_003
KINDS = (("dict_bool", 74), ("double", 24))


def test_reference_follows_java_min_max_and_fsum():
    nan, inf = math.nan, math.inf
    g = R.exact_groups([np.array([1, 1, 2, 2, 2, 3, 1])], [None], np.array([0.0, -0.0, 1e100, 1.0, -1e100, 5.0, nan]),
                       np.array([1, 1, 1, 1, 1, 0, 1], bool), np.array([1, 1, 1, 1, 1, 1, 0], bool))
    assert [x.key for x in g] == [(1,), (2,), (3,)] and [x.count for x in g] == [2, 3, 0] and [x.rows for x in g] == [2, 3, 1]
    assert math.copysign(1, g[0].min) == -1 and math.copysign(1, g[0].max) == 1 and not g[0].has_nan      # the NaN is filtered out
    assert g[1].sum == 1.0 and g[1].sum_abs == 2e100                          # fsum: exact, where a sequential sum gives 0.0
    assert g[2].min is None and g[2].max is None
    assert math.isnan(R.java_min(1.0, nan)) and math.isnan(R.java_max(nan, 1.0)) and R.java_min(inf, -inf) == -inf
    # keys follow Double.equals: NaNs are one group, -0.0 and 0.0 two, NULL its own
    k = np.array([nan, R.NAN_PAYLOAD, 0.0, -0.0, 7.0, 7.0])
    g = R.exact_groups([k], [np.array([1, 1, 1, 1, 1, 0], bool)], np.ones(6))
    assert [x.rows for x in g] == [2, 1, 1, 1, 1] and g[-1].key == (None,)
    assert R.sum_bound(0, 0.0) == 0.0 and R.sum_bound(1000, 1500.0) == pytest.approx(1000 * 2.0 ** -53 * 1500.0, rel=1e-12)
    assert R.avg_bound(3, 6.0) == pytest.approx(4 * 2.0 ** -53 * 2.0, rel=1e-12)


def test_check_aggregate_decides_the_special_cases():
    nan, inf = math.nan, math.inf

    def grp(vals):
        return R.exact_groups([], [], np.array(vals, dtype=np.float64))[0]

    def fails(fn, got, g):
        with pytest.raises(AssertionError):
            R.check_aggregate(fn, got, g)

    g = grp([1.0, nan, 2.0])
    for fn in (R.SUM, R.AVG, R.MIN, R.MAX):
        R.check_aggregate(fn, R.NAN_NEGATIVE, g)
        fails(fn, 3.0, g)
    g = grp([1.0, inf, -inf])
    R.check_aggregate(R.SUM, nan, g); R.check_aggregate(R.MIN, -inf, g); R.check_aggregate(R.MAX, inf, g)
    fails(R.SUM, inf, g)
    g = grp([1.0, -inf])
    R.check_aggregate(R.SUM, -inf, g); R.check_aggregate(R.AVG, -inf, g); fails(R.SUM, nan, g); fails(R.MAX, -inf, g)
    g = grp([-0.0, -0.0])
    R.check_aggregate(R.SUM, 0.0, g); R.check_aggregate(R.AVG, 0.0, g); R.check_aggregate(R.MIN, -0.0, g); R.check_aggregate(R.MAX, -0.0, g)
    fails(R.SUM, -0.0, g); fails(R.MIN, 0.0, g); fails(R.MAX, 0.0, g)
    g = grp([])
    for fn in (R.SUM, R.AVG, R.MIN, R.MAX):
        R.check_aggregate(fn, None, g)
        fails(fn, 0.0, g)
    R.check_aggregate(R.COUNT, 0.0, g); fails(R.COUNT, None, g); fails(R.COUNT, 1.0, g)
    g = grp([0.1, 0.2, 0.3])
    R.check_aggregate(R.SUM, 0.1 + 0.2 + 0.3, g); R.check_aggregate(R.SUM, 0.3 + 0.2 + 0.1, g); R.check_aggregate(R.AVG, (0.1 + 0.2 + 0.3) / 3, g)
    fails(R.SUM, 0.6 + 4 * 0.6 * 2.0 ** -53, g); fails(R.SUM, None, g); fails(R.SUM, inf, g); fails(R.COUNT, 2.0, g)
    # finite values that overflow in one order and not in another are an error of the test's input, not a skipped check
    with pytest.raises(ValueError):
        R.check_aggregate(R.SUM, 0.0, grp([R.DBL_MAX, -R.DBL_MAX, 1.0]))
    with pytest.raises(ValueError):
        R.check_aggregate(R.SUM, inf, grp([R.DBL_MAX / 2, R.DBL_MAX / 2, inf]))


def _cases(skewed_too=True):
    for name in R.DATASETS:
        for kind, ng in KINDS:
            yield name, kind, ng, False
    if skewed_too:
        yield "same_magnitude", "dict_bool", 74, True
        yield "wide_range", "double", 24, True


def test_special_groups_are_what_they_claim_to_be():
    """The compositions the `specials` data set promises exist, with and without the filter."""
    case = R.Case("dict", R.make_data("specials", N_ROWS, 24))
    for filtered in (False, True):
        g = {grp.key[0]: grp for grp in case.exact(filtered)["x"]}
        assert g[0].count > 1000 and g[0].sum_abs == 0.0 and math.copysign(1, g[0].max) == -1          # only -0.0
        assert math.copysign(1, g[1].min) == -1 and math.copysign(1, g[1].max) == 1 and g[1].sum_abs == 0.0
        assert g[2].has_nan and g[3].has_nan and g[4].has_nan and g[2].count > 1000
        assert g[5].has_pinf and not g[5].has_ninf and g[6].has_pinf and g[6].has_ninf and g[13].has_ninf and not g[13].has_pinf
        assert g[7].count == 0 and g[7].rows > 1000 and g[8].count == 1
        assert g[9].has_nan == (not filtered)                                   # the filter removes this group's only NaN
        r10 = case.data.x[(case.data.gid == 10) & case.data.x_valid & case.data.selected]
        assert (r10 == 5e-324).sum() == 1 and (r10 == -5e-324).sum() == 1 and g[10].sum_abs > 1e5 and g[11].max == R.DBL_MAX / 4 and g[12].min == -R.DBL_MAX / 4
        assert g[14].max == 5e-324 and g[14].min == -5e-324 and g[14].sum_abs < 1e-300
    x, gid, sel, valid = case.data.x, case.data.gid, case.data.selected, case.data.x_valid
    for grp, where in ((3, 0), (4, -1)):                                        # NaN as the first / the last valid row of its group
        r = np.nonzero((gid == grp) & sel & valid)[0]
        assert math.isnan(x[r[where]]) and not np.isnan(np.delete(x[r], where)).any()
    assert {int(np.array([x[np.nonzero((gid == g_) & sel & valid)[0][w]]]).view(np.uint64)[0]) for g_, w in ((3, 0), (4, -1))} == \
        {0x7ff8000000000123, 0xfff8000000000456}                               # two payloads, one with the sign bit set


@pytest.mark.parametrize("name,kind,ngroups,skewed", list(_cases()))
def test_oracle_is_within_the_bound_of_the_exact_reference(oracle, name, kind, ngroups, skewed):
    """The reference's own sequential order satisfies check_aggregate on every data set the GPU suite runs, at 200 003 rows
    behind dictionary x boolean and DOUBLE keys: the bound has room for a legitimate order.  Grouped and global."""
    data = R.make_data(name, N_ROWS, ngroups, skewed=skewed)
    case, glob = R.Case(kind, data), R.Case("none", data)
    for filtered in (False, True):
        rows = oracle.filter_groupby(case.cols, case.flt if filtered else None, case.keys, case.exprs, case.aggs, oracle.BYTECODE_COMPILER)
        assert len(rows) == ngroups
        worst = R.check_rows(case, filtered, rows, f"oracle, {name}, {kind} keys, filter {filtered}")
        vals, nsel = oracle.filter_aggregate(glob.cols, glob.flt if filtered else None, glob.exprs, glob.aggs, oracle.BYTECODE_COMPILER)
        assert nsel == glob.exact(filtered)["x"][0].rows
        worst = max(worst, R.check_rows(glob, filtered, [vals], f"oracle, {name}, global, filter {filtered}"))
        assert worst < 0.1            # a legitimate order uses a small part of the worst-case bound
        if name in ("wide_range", "same_magnitude") and not skewed:
            # the order of additions does matter on this data: the sequential sum differs from the exact one in the last bits
            differ = sum(r[len(case.keys)] != g.sum for r, g in zip(rows, case.exact(filtered)["x"]))
            assert differ > ngroups // 2
        if name == "subnormal":
            # integer multiples of 2^-1074: every order gives the exact sum
            for r, g in zip(rows, case.exact(filtered)["x"]):
                assert r[len(case.keys)] == g.sum and abs(g.sum) < 1e-300


def _gpu_batches():
    """(data set, distinct keys, rows, skewed) of every batch test_gpu_aggregate_numerics.py builds."""
    seen = []
    for route, (_, ng, n) in R.ROUTE_SHAPES.items():
        seen += [(name, ng, n, False) for name in R.DATASETS]
        if route in R.SKEWED_ROUTES:
            seen += [(name, ng, n, True) for name in ("same_magnitude", "wide_range")]
    seen += [(name, R.ROUTE_SHAPES[R.SIZES_ROUTE][1], n, False) for n in R.PARTITIONED_SIZES for name in R.SIZES_DATASETS]
    seen += [(name,) + R.GLOBAL_SHAPE + (False,) for name in R.DATASETS]
    return sorted(set(seen))


@pytest.mark.parametrize("name,ngroups,n,skewed", _gpu_batches())
def test_no_batch_of_the_gpu_suite_holds_an_undecidable_group(name, ngroups, n, skewed):
    """make_data seeds by (rows, keys): the batches the GPU routes run are other data than the 200 003-row ones above.  Every
    one of them is decidable -- per group and as a whole, for each aggregated expression, sum|x| stays below DBL_MAX / 2
    (checked without the filter: a filtered group is a subset) -- so check_aggregate never has to raise on the GPU."""
    data = R.make_data(name, n, ngroups, skewed=skewed)
    whole = [R.Case("none", data)] if (ngroups, n) == R.GLOBAL_SHAPE else []       # the global aggregate runs on these batches only
    for case in [R.Case("dict", data)] + whole:                         # (the kind of key does not change the groups)
        for groups in case.exact(False).values():
            for g in groups:
                R.decided_sum(g)
            assert sum(g.rows for g in groups) == n


def test_empty_selection_and_tiny_batches():
    """Data sets of 1 and 63 rows build, and an empty selection gives the one empty global group."""
    for n in (1, 63):
        for name in R.DATASETS:
            case = R.Case("dict", R.make_data(name, n, 5000))
            assert 1 <= len(case.exact(False)["x"]) <= n
    g = R.exact_groups([], [], np.array([1.0, 2.0]), None, np.zeros(2, bool))
    assert len(g) == 1 and g[0].count == 0 and g[0].rows == 0
    assert R.exact_groups([np.array([1, 2])], [None], np.array([1.0, 2.0]), None, np.zeros(2, bool)) == []


@pytest.mark.parametrize("skewed", [False, True])
def test_the_bound_sees_a_lost_a_doubled_and_a_misrouted_row(skewed):
    """On `same_magnitude` (|x| in [1, 2)) every value is more than twice the bound of its group -- also in the group that
    holds 90 % of the rows, whose bound is the widest -- so a SUM that lost a row, added one twice or added one into the
    neighbouring group fails check_aggregate."""
    data = R.make_data("same_magnitude", N_ROWS, 74, skewed=skewed)
    case = R.Case("dict", data)
    groups = case.exact(True)["x"]
    assert len(groups) == 74 and max(g.count for g in groups) > (100_000 if skewed else 1000)
    for g in groups:
        assert g.min_abs > 2 * R.sum_bound(g.count, g.sum_abs) and g.min_abs > 2 * g.count * R.avg_bound(g.count, g.sum_abs)
    sel = data.selected & data.x_valid
    members = [data.x[sel & (data.gid == (73 if g.key[0] is None else g.key[0]))] for g in groups]      # (group id 73 is the NULL key)
    for i, g in enumerate(groups):
        vals, other = members[i], members[(i + 1) % len(groups)]
        plain = float(np.sum(vals))                                   # numpy's pairwise order: one more legitimate order
        R.check_aggregate(R.SUM, plain, g)
        R.check_aggregate(R.AVG, plain / g.count, g)
        for wrong in (float(np.sum(vals[1:])), float(np.sum(vals[:-1])),                       # a row lost
                      float(np.sum(np.concatenate([vals, vals[len(vals) // 2:len(vals) // 2 + 1]]))),    # a row added twice
                      float(np.sum(np.concatenate([vals, other[:1]]))),                      # the neighbour's row added here
                      plain - float(vals[len(vals) // 3])):                                     # ... and this one's row added there
            with pytest.raises(AssertionError):
                R.check_aggregate(R.SUM, wrong, g)
            with pytest.raises(AssertionError):
                R.check_aggregate(R.AVG, wrong / g.count, g)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["wide_range", "same_magnitude", "cancelling", "specials", "subnormal"])
def test_sharded_merge_of_oracle_partials_is_within_the_bound(oracle, name, world):
    """expand_partial_aggregates -> per-shard partials (the oracle stands in for the GPU) -> merge_group_partials /
    combine_aggregate_partials -> finish_partials, over 64-row aligned shard ranges: groups in global first-appearance order,
    every aggregate within check_aggregate of the exact reference; groups that a shard does not hold, shards without rows, NaN,
    -0.0 and all-NULL groups included."""
    from queryengine_amd import Column
    for n in (300, 20_011):
        data = R.make_data(name, n, 74)
        case, glob = R.Case("dict_bool", data), R.Case("none", data)
        fns, src, recipe = Dist.expand_partial_aggregates(case.aggs)
        nk = len(case.keys)
        per_rank_groups, per_rank_global, sizes, absent = [], [], [], 0
        for rank in range(world):
            b, e = Dist.shard_range(n, rank, world)
            assert b % 64 == 0 or b == n
            sizes.append(e - b)
            cols = [Column(c.type, c.data[b:e], None if c.valid is None else c.valid[b:e], c.dictionary) for c in case.cols]
            rows = oracle.filter_groupby(cols, case.flt, case.keys, [case.exprs[i] for i in src], fns, oracle.BYTECODE_COMPILER) if e > b else []
            per_rank_groups.append([(tuple(r[:nk]), list(r[nk:])) for r in rows])
            absent += len(case.exact(True)["x"]) - len(rows)
            vals, _ = oracle.filter_aggregate(cols[nk:], glob.flt, [glob.exprs[i] for i in src], fns, oracle.BYTECODE_COMPILER)
            per_rank_global.append(vals)
        assert sum(sizes) == n
        if world == 8 and n == 300:
            assert absent > 8 * 74 - 300 and sizes[0] == 64 and sizes[-1] == 0         # groups missing from a shard; whole shards without rows
        merged = Dist.merge_group_partials(fns, per_rank_groups)
        rows = [list(k) + Dist.finish_partials(case.aggs, recipe, acc) for k, acc in merged]
        R.check_rows(case, True, rows, f"{name}, {world} shards of {n} rows")
        total = Dist.finish_partials(glob.aggs, recipe, Dist.combine_aggregate_partials(fns, per_rank_global))
        R.check_rows(glob, True, [total], f"{name}, global, {world} shards of {n} rows")
