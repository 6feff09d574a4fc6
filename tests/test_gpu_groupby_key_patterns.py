"""GROUP BY under PLACED keys (groupby_key_pattern_reference.py): keys computed from the inverted hashes so that they fill
the 32-slot probe window of a workgroup's LDS table, wrap the end of a table, exhaust the 4096-slot probe limit, overflow a
hash partition, sit on the half-full and 5/8-full thresholds, or leave a scatter tile's runs one record short of, equal to or
one past a line -- branches of the generated code that random keys under a good hash reach only by accident.

Every pattern runs three times on a plan of its own; every execution is compared with the reference (keys and order exact,
COUNT / SUM / MIN / MAX exact on integer-valued inputs, AVG by the 1e-12 rule of helpers.assert_group_columns_equal) AND its
qe_ctx_last_groupby_stats with what the reference predicts for that execution: the route that produced the result, the
launches abandoned on the way, the capacity that sufficed, the partitions.  A placement whose effect the stats cannot show is
not in this file.  test_groupby_key_patterns_cpu.py proves the placements and the comparison on the CPU.

The predicted stats are those of the 1st, 2nd and 3rd execution of a FRESH plan (use_ids, id_capacity, hash_capacity,
known_keys and hp_failed stick to a plan), so every pattern has a context of its own for its three
executions; the patterns of a route share schema, aggregates and tuning word, i.e. generated source: the code objects of a
route are compiled once and come from the JIT's cache afterwards."""
import pytest

import groupby_key_pattern_reference as G
import helpers as H
from queryengine_amd import native as N

pytestmark = pytest.mark.gpu

FORMS = {"hashed": N.FORM_GROUPBY_HASHED, "dense_ids": N.FORM_GROUPBY_HASHED, "dense_key_range": N.FORM_GROUPBY_DENSE,
         "hash_partitioned_host": N.FORM_GROUPBY_HASH_PARTITIONED, "hash_partitioned_device": N.FORM_GROUPBY_HASH_PARTITIONED}


def _run(name, stats_of_executions):
    """The pattern on a fresh context, once per entry of `stats_of_executions`: result and stats asserted every time."""
    from queryengine_amd import engine as E
    p = G.patterns()[name]
    word = G.ROUTE_WORDS[p.route]
    ctx = E.Context(device=0, tuning=[0, 0, 0, 0, 0, word, 0, 0] if word else [])
    try:
        batch = E.DeviceBatch.from_columns(ctx, p.cols)
        try:
            keys, exprs = [ctx.compile(k) for k in p.key_exprs], [ctx.compile(e) for e in p.agg_exprs]
            seen = []
            for rep, predicted in enumerate(stats_of_executions):
                res = E.filter_groupby(ctx, batch, None, keys, exprs, G.AGGS)
                got = res.to_columns()
                res.free()
                st = ctx.last_groupby_stats()
                seen.append(st)
                print(f"GROUPBY_KEY_PATTERN {name} execution {rep + 1}: {st}")
                what = f"pattern {name} (route {p.route}), execution {rep + 1}"
                H.assert_group_columns_equal(got, p.want, p.nkeys, G.AGGS, int(G.AF.AVG), what)
                assert st == predicted, f"{what}: stats {st}, predicted {predicted} (executions so far: {seen})"
                assert ctx.last_form == FORMS[st["route"]], f"{what}: form {ctx.last_form} under route {st['route']}"
        finally:
            batch.free()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", G.PATTERN_NAMES)
def test_group_by_under_placed_keys(native_lib, name):
    """Three executions of the pattern: the reference's groups in its order and the predicted stats, every time."""
    _run(name, G.patterns()[name].stats)


@pytest.mark.parametrize("layout", ["lines", "records"])
def test_hash_partition_overflow_is_not_repeated_by_later_executions(native_lib, layout):
    """A hash-partitioned attempt sized from an exact key count that overflows would choose the same partitions from the same
    count again: before run_groupby_hashed_route gave the form up when the fallback's count sizes the very partitions that have
    just overflowed, every later execution of such a plan repeated count pass, scatter pass and the abandoned aggregation (1
    abandoned launch on every execution).  300 keys that share the top 10 bits of the partition hash overflow 64 partitions on
    the first execution and the 256 sized from their count on the second: from the third execution on nothing is abandoned."""
    st = G.patterns()[f"hp_{layout}_overflow_at_every_partition_count"].stats
    assert [s["abandoned"] for s in st] == [2, 1, 0]
    _run(f"hp_{layout}_overflow_at_every_partition_count", st + [st[2], st[2]])
