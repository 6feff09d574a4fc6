"""One compiled plan over a stream of batches whose data changes between executions (the call sequence of INTEGRATION.md).

A plan is cached on schema, expressions and geometry -- not on data -- and remembers what earlier batches looked like
(Plan in qe_internal.h): the share of rows it kept, whether a chunk of the local form overflowed, the conjunct order it measured,
whether its keys fitted the LDS tables, the sizes of the id table and of the global hash table that sufficed, the number of
groups, whether the hash-partitioned form failed.  Every test here runs ONE context and ONE set of compiled expressions over
batches for which that memory is wrong -- in two orders, with an empty batch and a batch whose filter keeps nothing once the
state is set -- and compares EVERY execution with the CPU oracle on the whole batch: filter+project bit for bit, group-by as
the same groups in insertion order with exact COUNT / MIN / MAX / SUM (integer-valued inputs) and AVG within 1e-12.

Each test also asserts that it crossed the threshold it is about: the oracle's group counts and kept fractions against the
constants of qe_api.cpp / qe_groupby.cpp (12 % dense, 60 % two-pass, 3 % local, 64 keys for ids, 32 768 keys in the first id
table, 4000 keys and 4 Mi rows for the hash-partitioned form, 8 Mi rows for the sample and the conjunct probe), and
ctx.last_form where the forms differ.

The group-by sequences run every step through TWO plans, the aggregation without a filter and with `y < 500` (the filter is
part of the plan key): executions alternate between them and each plan sees the whole sequence.  That the batches of a
sequence share a plan is asserted for filter+project (the generated source is the same for every batch, the empty one
included); for group-by it is the documented assumption: same column types, same nullability, no STRING column."""
import functools

import numpy as np
import pytest

from queryengine_amd import Column
from queryengine_amd import engine as E
from queryengine_amd import native as N

from helpers import D, I64, Fn, assert_columns_equal, assert_group_columns_equal, col, fn, group_rows_to_columns, num

pytestmark = pytest.mark.gpu

RING, TWO_PASS, DENSE, LOCAL = N.FORM_RING, N.FORM_TWO_PASS, N.FORM_DENSE, N.FORM_LOCAL
HASHED, HASH_PARTITIONED = N.FORM_GROUPBY_HASHED, N.FORM_GROUPBY_HASH_PARTITIONED
# qe_options.tuning[5] (DebugBit in qe_internal.h)
NEVER_DENSE, HASHED_GLOBAL_ATOMICS, FORCE_LOCAL, FORCE_HP, HP_RECORDS = 32768, 131072, 262144, 8388608, 33554432
# the constants the sequences are built around (qe_api.cpp, qe_groupby.cpp)
DENSE_FROM, TWO_PASS_FROM, LOCAL_UPTO, SAMPLE_FROM_ROWS = 0.12, 0.6, 0.03, 8 << 20
IDS_FROM_KEYS, ID_TABLE_FILLS_FROM, HP_FROM_KEYS, HP_FROM_ROWS = 64, 32768, 4000, 4 << 20


def _nullable(column, valid):
    """`column` with a validity mask whatever the mask says: Column drops a mask without a NULL, and a batch without a mask binds
    a schema without nulls -- another plan.  The short and the empty batches of a nullable column keep theirs this way, as a host
    does that hands over the validity buffers of its stream."""
    column.valid = np.ascontiguousarray(valid, dtype=np.bool_)
    return column


# ---- filter + project: SELECT rid, a + rid, c * 2.0 WHERE a < 100 AND c < 0.5 ---------------------------------------------------
A_, C_, R_ = col("a", 0, I64), col("c", 1, D), col("rid", 2, I64)
FP_FILTER = fn(Fn.AND, fn(Fn.CMP_LT, A_, num(100)), fn(Fn.CMP_LT, C_, num(0.5)))
FP_PROJECTIONS = [R_, fn(Fn.ADD, A_, R_), fn(Fn.MUL, C_, num(2.0))]
FP_ROWS = 300_001        # 73 dense tiles of 4096 rows and a ragged one of 993
BIG_ROWS = 9_000_017     # past the 8 Mi rows from which a plan samples its selectivity and probes its conjuncts
STRETCH = (3_000_000, 3_180_000)


def _fp_masks(name, n, nullable):
    """(rows on which `a < 100` passes, rows on which `c < 0.5` passes) of the named batch: functions of the row id, nothing
    random, so the kept fraction is fixed by construction."""
    rid = np.arange(n, dtype=np.int64)
    yes, no = np.ones(n, dtype=bool), np.zeros(n, dtype=bool)
    if name in ("all", "len1"):
        return yes, yes
    if name in ("none", "len1_none", "empty"):
        return no, yes
    if name == "sparse":                       # 0.2 %, evenly spread
        return rid % 500 == 0, rid % 4 == 0
    if name == "one":                          # one kept row, in the last ragged tile
        return rid == n - 2, yes
    if name in ("len63", "len1025"):           # one row in 16
        return rid % 16 == 0, yes
    if name == "p1":
        return rid % 100 == 0, yes
    # either side of the 12 % line; a NULL c (one row in seven of the nullable variant) drops its row
    if name == "p13":
        return rid % 100 < (16 if nullable else 13), yes
    if name == "p11":
        return rid % 100 < (13 if nullable else 11), yes
    if name == "big_a":                        # `a < 100` passes 10 %, `c < 0.5` passes 50 %
        return rid % 10 == 0, (rid // 3) % 2 == 0
    if name == "big_b":                        # the rates swapped: 95 % and 2 %, the 2 % in ONE dense stretch
        return rid % 20 != 0, (rid >= STRETCH[0]) & (rid < STRETCH[1])
    raise KeyError(name)


_FP_ROWS_OF = {"len1": 1, "len1_none": 1, "len63": 63, "len1025": 1025, "empty": 0, "big_a": BIG_ROWS, "big_b": BIG_ROWS}


class _FpBatch:
    def __init__(self, name, nullable):
        self.name, self.n = name, _FP_ROWS_OF.get(name, FP_ROWS)
        n = self.n
        pa, pc = _fp_masks(name, n, nullable)
        rid = np.arange(n, dtype=np.int64)
        a = np.where(pa, rid % 100, 100 + rid % 900).astype(np.int64)
        c = np.where(pc, (rid % 499) / 1000.0, 0.5 + (rid % 499) / 1000.0)
        self.cols = [Column(I64, a), _nullable(Column(D, c), rid % 7 != 3) if nullable else Column(D, c), Column(I64, rid)]
        self._want = None

    def want(self, oracle):
        if self._want is None:                 # once per batch, shared by every visit of every test
            self._want = oracle.filter_project(self.cols, FP_FILTER, FP_PROJECTIONS, oracle.BYTECODE_COMPILER)
        return self._want

    def kept(self, oracle):
        return len(self.want(oracle)[0])


@functools.lru_cache(maxsize=None)
def _fp_batch(name, nullable):
    return _FpBatch(name, nullable)


def _fp_model(mode, names, nullable, oracle):
    """choose_form (qe_api.cpp) for batches below 8 Mi rows: the form of every execution from the share of rows the execution
    before it kept.  `mode`: "default", "never_dense" or "force_local".  Only the batch "all" overflows a slot of the local form
    (a chunk is 1024 rows at least, a slot 512 at most; the others keep 66 rows of a 32 Ki-row chunk at most)."""
    sel, overflowed, out = -1.0, False, []
    for name in names:
        b = _fp_batch(name, nullable)
        if b.n == 0:                           # returns before a form is chosen; nothing is remembered
            out.append(None)
            continue
        if mode != "never_dense" and sel >= DENSE_FROM:
            form = DENSE
        elif sel >= TWO_PASS_FROM:
            form = TWO_PASS
        elif mode == "force_local" and not overflowed:
            form = LOCAL
            if name == "all":
                form, overflowed = RING, True
        else:
            form = RING
        out.append(form)
        sel = b.kept(oracle) / b.n
    return out


def _run_fp_sequence(oracle, tuning, nullable, names, want_forms, ctx=None):
    """Every batch of `names` in turn through ONE context and ONE set of compiled expressions; every execution against the
    oracle, bit for bit.  Returns (forms, results per step)."""
    own = ctx is None
    ctx = E.Context(device=0, tuning=tuning) if own else ctx
    dev, forms, results = {}, [], []
    try:
        cf, cp = ctx.compile(FP_FILTER), [ctx.compile(p) for p in FP_PROJECTIONS]
        for name in dict.fromkeys(names):
            dev[name] = E.DeviceBatch.from_columns(ctx, _fp_batch(name, nullable).cols)
        source = E.generated_source(ctx, dev[names[0]], cf, cp)
        for step, name in enumerate(names):
            b = _fp_batch(name, nullable)
            res = E.filter_project(ctx, dev[name], cf, cp)
            form = ctx.last_form if b.n else None
            count, got = res.count, res.to_columns()
            res.free()
            forms.append(form)
            results.append(got)
            want = b.want(oracle)
            what = f"step {step} ({name}), forms so far {forms}"
            assert count == len(want[0]), what
            for j, (g, w) in enumerate(zip(got, want)):
                assert_columns_equal(g, w, f"{what}, projection {j}")
        print(f"forms {list(zip(names, forms))}")
        assert forms == want_forms, list(zip(names, forms, want_forms))
        # the same plan, really: no batch of the sequence binds its schema another way (the empty one included)
        for name, d in dev.items():
            assert E.generated_source(ctx, d, cf, cp) == source, f"batch {name} has a plan of its own"
    finally:
        for d in dev.values():
            d.free()
        if own:
            ctx.close()
    return forms, results


def _assert_fp_fractions(oracle, nullable):
    """the kept fractions the sequences rely on, from the oracle alone"""
    frac = lambda name: _fp_batch(name, nullable).kept(oracle) / _fp_batch(name, nullable).n
    assert frac("all") >= 0.85 and frac("none") == 0.0 and 0.0 < frac("sparse") <= 0.003
    assert _fp_batch("one", nullable).kept(oracle) == 1 and _fp_batch("len1", nullable).kept(oracle) == 1
    assert _fp_batch("one", nullable).want(oracle)[0].data[0] >= FP_ROWS - FP_ROWS % 4096      # in the last, ragged tile
    assert DENSE_FROM <= frac("p13") < 0.15 and 0.09 < frac("p11") < DENSE_FROM
    assert 0.0 < frac("p1") < LOCAL_UPTO and 0.0 < frac("len1025") < DENSE_FROM and 0.0 < frac("len63") < DENSE_FROM
    assert FP_ROWS % 4096 != 0 and FP_ROWS < SAMPLE_FROM_ROWS


FP_SEQUENCES = {
    # 1. the local form and its stale chunk size: sized from nothing (1 sub-tile), from 0.2 % and from 0 % (32 sub-tiles), then a
    #    batch that keeps everything overflows every slot, the same execution answers through the ring and the plan never tries again
    "local": (FORCE_LOCAL, "force_local",
              ["sparse", "sparse", "len1025", "len63", "len1_none", "empty", "none", "all", "sparse", "sparse", "none", "len1", "all"]),
    "local_reversed": (FORCE_LOCAL, "force_local",
                       ["all", "sparse", "sparse", "none", "empty", "all", "len1025", "len63", "len1", "sparse", "none"]),
    # 2. dense learned from a batch that keeps everything, then nothing / one row in the ragged tile / a one-row batch through
    #    the dense kernel, the ring after each of them, then 13 % and 11 % alternating across the 12 % line
    "dense": (0, "default",
              ["all", "all", "none", "all", "one", "all", "len1", "p13", "p11", "p13", "p11", "p13", "empty", "p11", "sparse", "none", "all"]),
    "dense_reversed": (0, "default",
                       ["p11", "p13", "p11", "p13", "p11", "all", "none", "empty", "all", "one", "all", "len1", "all", "all"]),
    # 3. two-pass learned (the dense form switched off)
    "two_pass": (NEVER_DENSE, "never_dense", ["all", "p1", "empty", "all", "all", "none", "p1"]),
    "two_pass_reversed": (NEVER_DENSE, "never_dense", ["p1", "all", "p1", "empty", "none", "all", "all", "len1", "one"]),
}


@pytest.mark.parametrize("nullable", [False, True], ids=["c_not_null", "c_nullable"])
@pytest.mark.parametrize("sequence", list(FP_SEQUENCES))
def test_filter_project_plan_over_changing_batches(oracle, sequence, nullable):
    bits, mode, names = FP_SEQUENCES[sequence]
    _assert_fp_fractions(oracle, nullable)
    want_forms = _fp_model(mode, names, nullable, oracle)
    at = lambda name, k=0: [i for i, x in enumerate(names) if x == name][k]
    # the crossings each sequence is about (derived from the constants; the model must not drift away from them)
    if sequence == "local":
        assert want_forms[:5] == [LOCAL] * 5 and want_forms[at("none")] == LOCAL
        assert want_forms[at("all")] == RING                                   # overflowed, answered through the ring
        assert want_forms[at("all") + 1:at("all") + 3] == [DENSE, RING]        # `sparse` after 100 %, then never local again
    elif sequence == "local_reversed":
        assert want_forms[:3] == [RING, DENSE, RING] and LOCAL not in want_forms
    elif sequence == "dense":
        assert want_forms[:4] == [RING, DENSE, DENSE, RING]
        assert want_forms[at("one")] == DENSE and want_forms[at("len1")] == DENSE
        assert want_forms[at("p13"):at("p13") + 5] == [DENSE, DENSE, RING, DENSE, RING]
    elif sequence == "dense_reversed":
        assert want_forms[:5] == [RING, RING, DENSE, RING, DENSE]
        assert want_forms[at("none")] == DENSE and want_forms[at("one")] == DENSE and want_forms[at("len1")] == DENSE
    else:
        assert want_forms[at("all") + 1] == TWO_PASS and DENSE not in want_forms
        assert want_forms.count(TWO_PASS) >= 2 and want_forms.count(RING) >= 3
    _run_fp_sequence(oracle, [0, 0, 0, 0, 0, bits], nullable, names, want_forms)


def test_conjunct_order_and_selectivity_from_another_distribution(oracle):
    """4. 9 M rows.  Batch A decides the conjunct order (`a < 100` passes 10 %, `c < 0.5` 50 %: as written) and leaves 6.7 % as the
    plan's selectivity; batch B has the rates swapped (95 % / 2 %) and its kept rows in ONE dense stretch.  The context that
    learned on A runs B in A's order and with A's selectivity; a fresh context that sees B first orders the other way round,
    samples 1.9 %, tries the local form and overflows its slots.  Both give the oracle's rows on every execution (the WHOLE batch
    is walked by the oracle), hence the same bytes as each other."""
    a, b = _fp_batch("big_a", False), _fp_batch("big_b", False)
    assert a.n == b.n >= SAMPLE_FROM_ROWS and a.n % 4096 != 0
    rate = lambda batch, k: float(np.mean(_fp_masks(batch.name, batch.n, False)[k]))
    assert abs(rate(a, 0) - 0.10) < 1e-3 and abs(rate(a, 1) - 0.50) < 1e-3
    assert abs(rate(b, 0) - 0.95) < 1e-3 and abs(rate(b, 1) - 0.02) < 1e-3
    assert LOCAL_UPTO < a.kept(oracle) / a.n < DENSE_FROM and 0.015 < b.kept(oracle) / b.n < LOCAL_UPTO
    rid_b = b.want(oracle)[0].data
    assert rid_b[0] >= STRETCH[0] and rid_b[-1] < STRETCH[1]                   # one dense stretch
    results = {}
    for label, names, want_forms, first_order in (
            # A: sampled 6.7 % -> ring.  B: ring (6.7 % remembered), leaves 1.9 %; the small batches leave 0 %; B again: local form with
            # the largest chunks, overflows in the stretch -> ring, and never again
            ("learned_on_a", ["big_a", "big_b", "empty", "none", "big_b", "big_a", "big_b"], [RING, RING, None, RING, RING, RING, RING], [0, 1]),
            # B first: sampled ~2 % -> local form, overflows -> ring
            ("learned_on_b", ["big_b", "big_a", "none", "empty", "big_b", "big_a"], [RING, RING, RING, None, RING, RING], [1, 0])):
        ctx = E.Context(device=0)
        try:
            cf, cp = ctx.compile(FP_FILTER), [ctx.compile(p) for p in FP_PROJECTIONS]
            probe = E.DeviceBatch.describe(ctx, a.cols)
            assert E.conjunct_order(ctx, probe, cf, cp) is None
            _, res = _run_fp_sequence(oracle, [], False, names, want_forms, ctx=ctx)
            assert E.conjunct_order(ctx, probe, cf, cp) == first_order, label   # decided by the first large batch, kept for good
            results[label] = {name: r for name, r in zip(names, res)}           # (the last visit of each batch)
            probe.free()
        finally:
            ctx.close()
    for name in ("big_a", "big_b"):
        for j, (g, w) in enumerate(zip(results["learned_on_a"][name], results["learned_on_b"][name])):
            assert_columns_equal(g, w, f"{name}: the two contexts, projection {j}")


# ---- group-by: SELECT k, SUM(x), MIN(x), MAX(x), COUNT(x), AVG(x), SUM(y + y) [WHERE y < 500] GROUP BY k ----------------------
GB_ROWS, GB_ROWS_WIDE = 250_003, 600_011
HEAVY_ROWS = 4_300_003    # the skew test of run_groupby_hp looks at batches of more than 2^22 kept records only
SELF_ROWS = (4 << 20) + 17

_GB = {   # name: (rows, distinct keys drawn from, seed, what is special)
    "k10": (GB_ROWS, 10, 1, None), "k5000": (GB_ROWS, 5000, 2, None), "k40000": (GB_ROWS, 40_000, 3, None),
    "null_keys": (GB_ROWS, 10, 4, "null_keys"), "nothing_kept": (GB_ROWS, 100, 5, "nothing_kept"), "empty": (0, 10, 6, None),
    "w100": (GB_ROWS_WIDE, 100, 7, None), "w150000": (GB_ROWS_WIDE, 150_000, 8, None), "w200000": (GB_ROWS_WIDE, 200_000, 9, None),
    "heavy": (HEAVY_ROWS, 50_000, 10, "heavy"),
    "s30": (SELF_ROWS, 30, 11, None), "s60000": (SELF_ROWS, 60_000, 12, None), "s60000_3pct": (SELF_ROWS, 60_000, 13, "3pct"),
}


class _GbBatch:
    def __init__(self, name, kt):
        n, nkeys, seed, special = _GB[name]
        rng = np.random.default_rng(seed)
        self.name, self.n, self.kt = name, n, kt
        if kt == D:
            pool = np.concatenate([[0.0, -0.0, float("nan")], rng.normal(0, 1e6, nkeys)])[:nkeys]
        else:
            pool = rng.integers(-2 ** 62, 2 ** 62, nkeys)
        pick = rng.integers(0, nkeys, n)
        if special == "heavy":             # one key owns 60 % of the rows, 50 000 share the rest
            pick = np.where(rng.random(n) < 0.6, 0, pick)
        k_valid = rng.random(n) > 0.02 if special != "null_keys" else np.zeros(n, dtype=bool)
        self.key_rows = np.bincount(pick[k_valid], minlength=nkeys)             # rows of every key of the pool
        x = np.round(rng.normal(0, 100, n))                                    # integer valued: sums are exact in any order
        y = rng.integers(-1000, 1000, n)
        if special == "nothing_kept":
            y = rng.integers(500, 1000, n)
        elif special == "heavy":           # the filter keeps every row: more than 2^22 records with and without it
            y = rng.integers(-1000, 500, n)
        elif special == "3pct":
            y = np.where(rng.random(n) < 0.03, y % 500, 500 + y % 500)
        self.cols = [_nullable(Column(kt, pool[pick].astype(np.float64 if kt == D else np.int64)), k_valid),
                     _nullable(Column(D, x), rng.random(n) > 0.2), Column(I64, y.astype(np.int64))]
        self._want = {}

    def want(self, oracle, filtered):
        if filtered not in self._want:         # once per batch and plan, as columns, shared by every visit of every test
            keys, exprs, aggs, flt = _gb_query(self.kt, oracle)
            rows = oracle.filter_groupby(self.cols, flt if filtered else None, keys, exprs, aggs, oracle.BYTECODE_COMPILER)
            self._want[filtered] = group_rows_to_columns(rows, [self.kt], len(aggs))
        return self._want[filtered]

    def groups(self, oracle, filtered):
        return len(self.want(oracle, filtered)[0])


@functools.lru_cache(maxsize=None)
def _gb_batch(name, kt):
    return _GbBatch(name, kt)


def _gb_query(kt, oracle):
    K, X, Y = col("k", 0, kt), col("x", 1, D), col("y", 2, I64)
    return ([K], [X, X, X, X, X, fn(Fn.ADD, Y, Y)], [oracle.SUM, oracle.MIN, oracle.MAX, oracle.COUNT, oracle.AVG, oracle.SUM],
            fn(Fn.CMP_LT, Y, num(500)))


def _run_gb_sequence(oracle, bits, kt, steps):
    """`steps`: (batch, form -- or (form without the filter, form with it), or None) in turn through ONE context and ONE set of
    compiled expressions, each step through the plan without a filter and then through the plan with `y < 500`; every execution
    against the oracle."""
    keys, exprs, aggs, flt = _gb_query(kt, oracle)
    ctx = E.Context(device=0, tuning=[0, 0, 0, 0, 0, bits])
    dev, forms = {}, []
    try:
        ck, ce, cf = [ctx.compile(k) for k in keys], [ctx.compile(e) for e in exprs], ctx.compile(flt)
        for name, _ in steps:
            if name not in dev:
                dev[name] = E.DeviceBatch.from_columns(ctx, _gb_batch(name, kt).cols)
        for step, (name, want_form) in enumerate(steps):
            for filtered in (False, True):
                res = E.filter_groupby(ctx, dev[name], cf if filtered else None, ck, ce, aggs)
                forms.append(ctx.last_form)
                got = res.to_columns()
                res.free()
                what = f"step {step} ({name}{', y < 500' if filtered else ''}), forms so far {forms}"
                assert_group_columns_equal(got, _gb_batch(name, kt).want(oracle, filtered), 1, aggs, oracle.AVG, what)
                want = want_form[int(filtered)] if isinstance(want_form, tuple) else want_form
                assert want is None or forms[-1] == want, what
        print(f"forms {[(name, forms[2 * i], forms[2 * i + 1]) for i, (name, _) in enumerate(steps)]}")
    finally:
        for d in dev.values():
            d.free()
        ctx.close()
    return forms


def _assert_gb_counts(oracle, kt):
    """the group counts the sequences rely on, with and without the filter, from the oracle alone"""
    for filtered in (False, True):
        g = lambda name: _gb_batch(name, kt).groups(oracle, filtered)
        assert 1 < g("k10") <= IDS_FROM_KEYS and IDS_FROM_KEYS < g("k5000") <= ID_TABLE_FILLS_FROM < g("k40000")
        assert g("null_keys") == 1 and g("empty") == 0 and g("nothing_kept") == (0 if filtered else 101)
        assert not _gb_batch("null_keys", kt).cols[0].valid.any()
    for name in ("k10", "k5000", "k40000", "w100"):
        assert _gb_batch(name, kt).n % 4096 != 0 and _gb_batch(name, kt).n < HP_FROM_ROWS


@pytest.mark.parametrize("order", ["few_first", "many_first"])
@pytest.mark.parametrize("kt", [D, I64], ids=["double_key", "int64_key"])
def test_hashed_group_by_lds_tables_then_ids_and_back(oracle, kt, order):
    """5. 10 keys stay in the workgroups' LDS tables; 5000 do not fit them: the id build runs inside that execution and from then
    on, also on 10 keys, on a batch whose every key is NULL and on an empty one; 40 000 keys fill the remembered first id table
    (more than half of 65 536 entries), which grows four-fold and is then remembered too large for what follows."""
    _assert_gb_counts(oracle, kt)
    names = {"few_first": ["k10", "k5000", "k10", "k40000", "k10", "empty", "null_keys", "nothing_kept", "k5000", "k10"],
             "many_first": ["k40000", "k10", "k40000", "nothing_kept", "empty", "k5000", "null_keys", "k10", "k40000"]}[order]
    _run_gb_sequence(oracle, 0, kt, [(name, HASHED) for name in names])


@pytest.mark.parametrize("order", ["few_first", "many_first"])
@pytest.mark.parametrize("kt", [D, I64], ids=["double_key", "int64_key"])
def test_hashed_group_by_remembered_global_table(oracle, kt, order):
    """6. the global-atomic form (debug bit 131072): ~190 000 keys use more than half of the first table of 65 536 entries, the
    table grows eight-fold within the execution and that capacity is what 100 keys meet next; the other way round the small table
    of the 100 keys meets the many."""
    for filtered in (False, True):
        assert _gb_batch("w200000", kt).groups(oracle, filtered) > 65536 // 2
        assert IDS_FROM_KEYS < _gb_batch("w100", kt).groups(oracle, filtered) < 200
    names = {"few_first": ["w100", "w200000", "w100", "empty", "nothing_kept", "w200000", "w100"],
             "many_first": ["w200000", "w100", "w200000", "nothing_kept", "empty", "w100"]}[order]
    _run_gb_sequence(oracle, HASHED_GLOBAL_ATOMICS, kt, [(name, HASHED) for name in names])


@pytest.mark.parametrize("kt,layout,order", [(D, "lines", "few_first"), (I64, "lines", "many_first"),
                                             (I64, "records", "few_first"), (D, "records", "many_first")],
                         ids=["double_key-lines-few_first", "int64_key-lines-many_first", "int64_key-records-few_first",
                              "double_key-records-many_first"])
def test_forced_hash_partitioned_group_by_over_changing_key_counts(oracle, kt, layout, order):
    """7. the hash-partitioned form from the first execution on (debug bit 8388608; "records": the {header, words} layout).  Its
    partition count and bucket shift come from the group count of the execution before: the 64 x 256 or 256 x 256 buckets that fit
    100 keys cannot hold ~147 000 (fewer buckets than keys), that execution falls back to the hashed form and reports the count;
    the next one has 512 x 1024 buckets; 100 keys then sit in those.  A heavy-hitter batch -- one key owns 60 % of 4.3 M rows, the
    smallest batch whose kept records pass the 2^22 below which run_groupby_hp does not look for skew, with and without the
    filter -- makes the plan give the form up for good."""
    for filtered in (False, True):
        g = lambda name: _gb_batch(name, kt).groups(oracle, filtered)
        assert g("w150000") > 256 * 256 and g("w150000") * 2 <= 512 * 1024      # overflows 256 partitions x 256 buckets, fits 512 x 1024
        assert IDS_FROM_KEYS < g("w100") < 200 and g("heavy") > HP_FROM_KEYS
        heavy = _gb_batch("heavy", kt)
        w = heavy.want(oracle, filtered)
        count = w[1 + 3].data                                                   # COUNT(x) per group
        records = heavy.n                                                       # y < 500 on every row of this batch
        assert records > 1 << 22 and count.max() > 0.4 * records > 3 * (records // 64) + 65536    # skewed for every P >= 64
    assert _gb_batch("heavy", kt).cols[2].data.max() < 500
    HP = HASH_PARTITIONED
    steps = {"few_first": [("w100", HP), ("w150000", HASHED), ("w150000", HP), ("w100", HP), ("heavy", HASHED), ("w150000", HASHED),
                           ("empty", HASHED), ("nothing_kept", HASHED), ("w100", HASHED)],
             "many_first": [("w150000", HASHED), ("w150000", HP), ("w100", HP), ("w150000", HASHED), ("w150000", HP), ("empty", HASHED),
                            ("nothing_kept", None), ("w150000", HASHED), ("heavy", HASHED), ("w100", HASHED)]}[order]
    _run_gb_sequence(oracle, FORCE_HP | (HP_RECORDS if layout == "records" else 0), kt, steps)


@pytest.mark.parametrize("order", ["few_first", "many_first"])
def test_hash_partitioned_group_by_chosen_by_the_plan(oracle, order):
    """8. 4 Mi + 17 rows, default context: the plan itself turns to the hash-partitioned form once it has seen 4000 keys or more
    on a batch of 4 Mi rows or more.  After 30 keys, 60 000 keys grow the id table inside the hashed form (the plan is not new any
    more); the next execution is hash-partitioned, 256 partitions.  Then the 30 keys again, in those partitions.  The plan with
    the filter keeps 3.1 M records, fewer than the 2^22 from which run_groupby_hp looks for skew: hash-partitioned, 30 keys are
    left as the known count, the 60 000 keys under a filter that keeps 3 % run hashed and the next batch hash-partitioned again.
    The plan without a filter has 4 Mi + 17 records and every one of the 30 keys owns more of them than a partition may hold
    (3 shares of 1 / 256 + 65 536): skew, the form is given up for good.  A plan whose FIRST batch has the 60 000 keys goes
    hash-partitioned inside that execution (the first id table fills)."""
    kt = D
    assert SELF_ROWS >= HP_FROM_ROWS and SELF_ROWS % 4096 != 0
    for filtered in (False, True):
        g = lambda name: _gb_batch(name, kt).groups(oracle, filtered)
        assert 1 < g("s30") <= IDS_FROM_KEYS and g("s60000") > ID_TABLE_FILLS_FROM and g("s60000_3pct") > ID_TABLE_FILLS_FROM
        assert g("s60000") >= HP_FROM_KEYS and g("s60000_3pct") >= HP_FROM_KEYS
        assert g("s60000") * 10 <= (256 << 10) * 3                             # 256 partitions (run_groupby_hashed_route)
    y = _gb_batch("s60000_3pct", kt).cols[2].data
    assert 0.025 < float(np.mean(y < 500)) < 0.035
    few = _gb_batch("s30", kt)
    assert few.key_rows.min() > 3 * (SELF_ROWS // 256) + 65536 and SELF_ROWS > 1 << 22        # without the filter: skew, whatever the hash
    assert int(np.sum(few.cols[2].data < 500)) <= 1 << 22                      # with it: too few records for the skew test
    HP = HASH_PARTITIONED
    # (batch, form of the plan without the filter, form of the plan with it)
    steps = {"few_first": [("s30", HASHED), ("s60000", HASHED), ("s60000", HP), ("s30", (HASHED, HP)), ("s60000_3pct", HASHED),
                           ("s60000", (HASHED, HP)), ("empty", HASHED), ("nothing_kept", HASHED), ("s30", HASHED)],
             "many_first": [("s60000", HP), ("s30", (HASHED, HP)), ("s60000", HASHED), ("s60000_3pct", (HASHED, HP)), ("nothing_kept", HASHED),
                            ("empty", HASHED), ("s60000", HASHED), ("s30", (HASHED, HP))]}[order]
    _run_gb_sequence(oracle, 0, kt, steps)
