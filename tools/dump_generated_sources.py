#!/usr/bin/env python3
"""Dump every HIP source the fused-kernel generator produces for a fixed corpus of plans (no GPU needed).

The generator is a pure host function of its input, so a refactor of it can be proven text-preserving: run this tool in
two checkouts (each built with `make` in queryengine_amd/csrc) and compare the output directories,

    python tools/dump_generated_sources.py --out /tmp/a --jobs 16          (in checkout A)
    python tools/dump_generated_sources.py --out /tmp/b --jobs 16          (in checkout B)
    diff -r -x '*.hsaco' /tmp/a /tmp/b && echo identical

Per option set (tuning vector, comparison semantics) a planning-only context runs the corpus through prepare (default,
wide, mid and dense candidates), prepare_aggregate, prepare_groupby and generated_source, and leaves its JIT cache in
OUT/<option set>/: <hash>_<len>_gfx950.hip per compiled source, .rej per source rejected for spilling (the hash is of the
text, so equal file-name lists mean equal rejected sources too).  Plans that must FAIL write their code and message to
OUT/errors.txt.  Inputs that only executors with a device set (measured conjunct order, hash-partition shapes) go
through the C++ driver next to this file (dump_codegen_cases.cpp, linked against the checkout's libqe_hip.so) into
OUT/cases/.  With --seed DIR the caches start as copies of DIR's: sources that did not change are not compiled again.
"""
import argparse
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def option_sets():
    def t(**kw):
        v = [0] * 8
        for k, x in kw.items():
            v[int(k[1:])] = x
        return v
    sets = [("default_wl", [], 0, "wl"), ("default_fp", [], 0, "fp"), ("default_agg", [], 0, "agg"), ("default_gb", [], 0, "gb"),
            ("default_fail", [], 0, "fail"), ("ieee", [], 1, "wl fp"), ("hp", t(t5=8388608), 0, "gb"),
            ("hp_records", t(t5=8388608 | 33554432), 0, "gb"), ("dense", t(t5=16384), 0, "wl fp")]
    for d in (2, 3, 4, 5):
        sets.append((f"t2_{d}", t(t2=d), 0, "small"))
    for pm in (0, 1, 2, 3):
        sets.append((f"prio{pm}", t(t2=10 * (pm + 1)), 0, "small"))
    for bit in (2048, 4096, 2097152, 4194304, 33554432, 1, 2, 4, 16, 32, 64):
        sets.append((f"t5_{bit}", t(t5=bit), 0, "small"))
    sets += [("gate", t(t6=1 + 100 * 12 + 10000 * 6), 0, "small"), ("stagger", t(t7=1), 0, "small"), ("nostagger", t(t7=2), 0, "small"),
             ("resolve3", t(t7=13), 0, "small"), ("nbuf3", t(t7=300), 0, "small"),
             ("explicit", t(t0=128, t1=4, t3=302, t4=8 + 10000 * 2), 0, "small"), ("threads512", t(t0=512), 0, "small")]
    return sets


def run_option_set(repo, out, name, tuning, cmp, scope):
    sys.path.insert(0, repo)
    import numpy as np
    from queryengine_amd import (BooleanLiteralExpression, Column, ColumnExpression, DataType, Function, FunctionExpression,
                                 NumericLiteralExpression, StringLiteralExpression)
    from queryengine_amd import engine as E
    from queryengine_amd import native as N
    from queryengine_amd import workloads as W
    from queryengine_amd.prepared import _schema_columns
    D, I64, I32, B, S = DataType.DOUBLE, DataType.INT64, DataType.INT32, DataType.BOOLEAN, DataType.STRING
    Fn = Function
    scope = scope.split()
    ctx = E.Context(device=None, jit_cache_dir=os.path.join(out, name), tuning=tuning, cmp_semantics=cmp)
    errors = []

    def fe(f, *ops, t=None):
        return FunctionExpression(f, list(ops), t) if t is not None else FunctionExpression(f, list(ops))

    def num(v):
        return NumericLiteralExpression(float(v))

    def comp(es):
        return [ctx.compile(e) for e in es]

    def fp(cols, flt, projs, label=None):
        """filter+project: the source of the first candidate, then every candidate prepare builds"""
        def go():
            batch = E.DeviceBatch.describe(ctx, cols)
            cf = ctx.compile(flt) if flt is not None else None
            cp = comp(projs)
            E.generated_source(ctx, batch, cf, cp)
            E.prepare(ctx, batch, cf, cp)
        attempt(go, label)

    def agg(cols, flt, exprs, aggs, label=None):
        attempt(lambda: E.prepare_aggregate(ctx, E.DeviceBatch.describe(ctx, cols), ctx.compile(flt) if flt is not None else None,
                                            comp(exprs), aggs), label)

    def gb(cols, flt, keys, exprs, aggs, label=None):
        attempt(lambda: E.prepare_groupby(ctx, E.DeviceBatch.describe(ctx, cols), ctx.compile(flt) if flt is not None else None,
                                          comp(keys), comp(exprs), aggs), label)

    def attempt(fn, label):
        try:
            fn()
            if label:
                errors.append(f"{name}/{label}: no error")
        except N.QeError as e:
            if not label:
                raise
            errors.append(f"{name}/{label}: {e.code} {e}")

    nul = np.array([True, False])
    dcol = lambda nullable=False: Column(D, np.zeros(2), nul if nullable else None)
    icol = lambda nullable=False: Column(I64, np.zeros(2, dtype=np.int64), nul if nullable else None)
    i32col = lambda nullable=False: Column(I32, np.zeros(2, dtype=np.int32), nul if nullable else None)
    bcol = lambda nullable=False: Column(B, np.zeros(2, dtype=np.bool_), nul if nullable else None)
    scol = lambda d, nullable=False: Column(S, np.zeros(2, dtype=np.int32), nul if nullable else None, list(d))

    # ---- filter + project ----
    wls = [W.config1(1000), W.config2(1000), W.config2(1000, null_pct=1), W.config3(1000), W.config4(1000), W.config2_swapped(1000)]
    if "small" in scope:
        wls = [W.config2(1000), W.config2(1000, null_pct=1), W.config3(1000)]
    if "wl" in scope or "small" in scope:
        for wl in wls:
            fp(_schema_columns(wl), wl.filter, wl.projections)
    a, b, c = ColumnExpression("a", 0, D), ColumnExpression("b", 1, I64), ColumnExpression("c", 2, I32)
    p, s, s2 = ColumnExpression("p", 3, B), ColumnExpression("s", 4, S), ColumnExpression("s2", 5, S)
    d1, d2 = ["pear", "apple", "fig"], ["kiwi", "apple", "\U0001F34E", ""]
    for nullable in ((False, True) if "fp" in scope else ()):
        cols = [dcol(nullable), icol(nullable), i32col(nullable), bcol(nullable), scol(d1, nullable), scol(d2, nullable)]
        fp(cols, None, [a, b, c, p, s])                                                     # no filter, every type out
        fp(cols, fe(Fn.CMP_LT, a, num(1)), [fe(Fn.ADD, a, b), fe(Fn.UNARY_MINUS, c), fe(Fn.NOT, p)])   # one conjunct
        fp(cols, p, [fe(Fn.MOD, b, b), fe(Fn.DIV, c, c), fe(Fn.MOD, a, a), fe(Fn.UNARY_PLUS, a), fe(Fn.UNARY_MINUS, b), fe(Fn.UNARY_MINUS, a)])
        fp(cols, fe(Fn.AND, fe(Fn.OR, p, fe(Fn.CMP_GE, a, b)), fe(Fn.CMP_NE, c, num(3))),
           [fe(Fn.IF, p, a, num(2)), fe(Fn.SUB, b, c), fe(Fn.MUL, c, c), fe(Fn.DIV, a, num(3)), fe(Fn.CMP_EQ, p, BooleanLiteralExpression(True))])
        # strings: ranks across dictionaries, against literals, literal against literal, IF over strings, SELECT 'lit'
        fp(cols, fe(Fn.AND, fe(Fn.CMP_LT, s, s2), fe(Fn.CMP_GE, s, StringLiteralExpression("b"))),
           [fe(Fn.IF, p, s, s2), fe(Fn.IF, p, s, StringLiteralExpression("none")), fe(Fn.IF, p, StringLiteralExpression("x"), StringLiteralExpression("y")),
            StringLiteralExpression("lit"), fe(Fn.CMP_EQ, s, s2), fe(Fn.CMP_EQ, s, s), fe(Fn.CMP_NE, s, StringLiteralExpression("fig")),
            fe(Fn.CMP_LT, StringLiteralExpression("a"), StringLiteralExpression("b")), fe(Fn.CMP_EQ, StringLiteralExpression("zz"), s2)])
        # DOUBLE comparisons of every flavour (literal on either side, zero / NaN-prone operands, integer shortcut)
        fp(cols, fe(Fn.AND, fe(Fn.AND, fe(Fn.AND, fe(Fn.CMP_LT, a, num(0)), fe(Fn.CMP_GT, num(2.5), a)), fe(Fn.CMP_LE, a, a)),
                    fe(Fn.AND, fe(Fn.CMP_GE, b, num(7)), fe(Fn.CMP_GT, num(7), b))),
           [fe(Fn.CMP_EQ, a, a), fe(Fn.CMP_NE, a, num(0)), fe(Fn.CMP_EQ, a, num(1.5)), fe(Fn.CMP_GT, a, num(2.5)), fe(Fn.CMP_GE, a, num(2.5)),
            fe(Fn.CMP_LE, a, num(2.5)), fe(Fn.CMP_LT, num(2.5), a), fe(Fn.CMP_LE, num(2.5), a), fe(Fn.CMP_GE, num(2.5), a), fe(Fn.CMP_LT, p, p),
            fe(Fn.CMP_LT, b, c), fe(Fn.CMP_EQ, b, num(3)), fe(Fn.OR, p, fe(Fn.CMP_LT, a, num(1))), fe(Fn.AND, p, fe(Fn.NOT, p))])
        fp(cols, fe(Fn.CMP_LT, a, num(1)), [fe(Fn.ADD, a, num(i)) for i in range(16)])      # wide enough to halve threads / unroll
        # null tests over a column and over an expression, as filter conjuncts and as projections; columns that only null tests read
        lit = StringLiteralExpression
        fp(cols, fe(Fn.AND, fe(Fn.IS_NOT_NULL, a), fe(Fn.IS_NULL, fe(Fn.ADD, b, c))),
           [fe(Fn.IS_NULL, a), fe(Fn.IS_NOT_NULL, s), fe(Fn.IS_NULL, fe(Fn.ADD, a, b)), fe(Fn.IS_NOT_NULL, fe(Fn.CMP_LT, s, s2)), fe(Fn.IS_NULL, num(1)), b])
        fp(cols, fe(Fn.IS_NULL, p), [fe(Fn.IS_NOT_NULL, c), fe(Fn.IS_NULL, s2)])
        # COALESCE over numeric, BOOLEAN and STRING operands: one dictionary, two, column against literal (present / absent), literal first
        fp(cols, fe(Fn.COALESCE, p, fe(Fn.CMP_LT, a, num(1))),
           [fe(Fn.COALESCE, a, b), fe(Fn.COALESCE, c, num(0)), fe(Fn.COALESCE, b, c), fe(Fn.COALESCE, p, BooleanLiteralExpression(False)),
            fe(Fn.COALESCE, s, s), fe(Fn.COALESCE, s, s2), fe(Fn.COALESCE, s, lit("none")), fe(Fn.COALESCE, s, lit("fig")),
            fe(Fn.COALESCE, lit("x"), s2), fe(Fn.COALESCE, lit("x"), lit("y")), fe(Fn.COALESCE, fe(Fn.IF, p, s, s2), lit("kiwi"))])
        fp(cols, fe(Fn.CMP_LT, fe(Fn.ABS, a), num(1)), [fe(f, x) for f in (Fn.ABS, Fn.FLOOR, Fn.CEIL) for x in (a, b, c)])
        # the integer shortcut of (double)int OP literal through identity nodes (unary plus, FLOOR of an integer), and what must not take it
        fp(cols, fe(Fn.CMP_LT, fe(Fn.UNARY_PLUS, b), num(7)),
           [fe(Fn.CMP_GE, num(3), fe(Fn.UNARY_PLUS, c)), fe(Fn.CMP_EQ, fe(Fn.FLOOR, b), num(2)), fe(Fn.CMP_LT, fe(Fn.ABS, c), num(2.0 ** 53)),
            fe(Fn.CMP_LE, b, num(2.0 ** 53 - 1)), fe(Fn.CMP_GT, b, num(-2.0 ** 53)), fe(Fn.CMP_LT, c, num(0.5))])
    if "small" in scope:
        cols = [dcol(True), icol(), i32col(), bcol(True), scol(d1), scol(d2)]
        fp(cols, fe(Fn.AND, p, fe(Fn.CMP_LT, a, num(1))), [a, p, s])
        fp(cols, None, [a, b])

    # ---- global aggregate ----
    if "agg" in scope or "small" in scope:
        every = [N.AGG_MIN, N.AGG_MAX, N.AGG_SUM, N.AGG_COUNT, N.AGG_AVG]
        for nullable in (False, True):
            cols = [dcol(nullable), icol(nullable), i32col(nullable)]
            agg(cols, None, [a, b, c, a, b], every)
            agg(cols, fe(Fn.AND, fe(Fn.CMP_LT, a, num(1)), fe(Fn.CMP_GT, b, num(5))), [a, b, c, a, b], every)
        wl = W.config2(1000)
        agg(_schema_columns(wl), wl.filter, wl.projections, [N.AGG_SUM, N.AGG_SUM])

    # ---- group by ----
    if "gb" in scope or "small" in scope:
        K, X, Y = ColumnExpression("k", 0, S), ColumnExpression("x", 1, D), ColumnExpression("y", 2, I64)
        K2, P = ColumnExpression("k2", 3, S), ColumnExpression("p", 4, B)
        flt = fe(Fn.CMP_LT, Y, num(5))
        sizes = (10, 2500, 100_000, 1_000_000) if "small" not in scope else (10, 100_000)
        for nkeys in sizes:
            cols = [scol(["k%07d" % i for i in range(nkeys)]), dcol(True), icol(), scol(["u", "v", "w"], True), bcol(True)]
            gb(cols, None, [K], [Y, Y], [N.AGG_SUM, N.AGG_COUNT])
            gb(cols, flt, [K], [X, Y, X], [N.AGG_SUM, N.AGG_MAX, N.AGG_AVG])
            gb(cols, fe(Fn.AND, flt, fe(Fn.CMP_GT, X, num(0))), [K, K2, P], [X, Y], [N.AGG_MIN, N.AGG_MAX])
        cols = [scol(["a", "b"]), dcol(), icol(), scol(["u", "v", "w"], True), bcol(True)]
        gb(cols, None, [P, StringLiteralExpression("lit")], [X], [N.AGG_AVG])
        gb(cols, None, [K], [fe(Fn.ADD, X, num(i)) for i in range(9)], [N.AGG_SUM] * 9)     # more than 8 aggregates
        gb([scol(["k%07d" % i for i in range(100_000)]), dcol(), icol(), scol(["u"]), bcol()], None, [K],
           [fe(Fn.ADD, X, num(i)) for i in range(9)], [N.AGG_SUM] * 9)                     # .. on a domain that does not fit LDS
        # hashed keys (with tuning[5] bit 8388608: their hash-partitioned plans)
        for nullable in (False, True):
            cols = [dcol(nullable), icol(nullable), dcol(nullable), i32col(nullable), scol(d1, nullable)]
            A, Bk, V, Ck, Sk = (ColumnExpression("a", 0, D), ColumnExpression("b", 1, I64), ColumnExpression("v", 2, D),
                                ColumnExpression("c", 3, I32), ColumnExpression("s", 4, S))
            gb(cols, None, [A], [V, V], [N.AGG_MIN, N.AGG_MAX])
            gb(cols, None, [Bk], [V, V, V], [N.AGG_SUM, N.AGG_COUNT, N.AGG_AVG])
            gb(cols, fe(Fn.CMP_LT, V, num(1)), [Ck], [V], [N.AGG_SUM])
            gb(cols, None, [A, Bk], [V], [N.AGG_SUM])
            gb(cols, None, [A, Bk, Ck, Sk], [V, Bk], [N.AGG_MAX, N.AGG_COUNT])
            gb(cols, None, [A, Bk, Ck, Sk, A], [V], [N.AGG_SUM])                           # five keys: no hash partitions
            gb(cols, None, [A], [fe(Fn.ADD, V, num(i)) for i in range(9)], [N.AGG_SUM] * 9)
            gb(cols, None, [A], [fe(Fn.ADD, V, num(i)) for i in range(6)], [N.AGG_AVG] * 6)   # wide records / entries

    # ---- plans that must fail ----
    if "fail" in scope:
        cols = [dcol(), icol(), scol(d1)]
        x0, s0 = ColumnExpression("a", 0, D), ColumnExpression("s", 2, S)
        fp(cols, None, [ColumnExpression("z", 7, D)], "column out of range")
        fp(cols, None, [ColumnExpression("a", 0, I64)], "wrong column type")
        fp(cols, x0, [x0], "non-BOOLEAN filter")
        agg(cols, None, [s0], [N.AGG_SUM], "aggregate over a string")
        gb(cols, None, [s0] * 9, [x0], [N.AGG_SUM], "9 group keys")
        fp(cols, None, [fe(Fn.ADD, x0, num(i)) for i in range(17)], "17 projections")
        many = [dcol(True) for _ in range(17)]
        fp(many, None, [fe(Fn.ADD, ColumnExpression("c", i, D), ColumnExpression("c", 16, D)) for i in range(16)], "17 input columns")
        sixteen = [dcol(True) for _ in range(16)]
        chain = ColumnExpression("c", 0, D)
        for i in range(1, 16):
            chain = fe(Fn.ADD, chain, ColumnExpression("c", i, D))
        fp([dcol(True) for _ in range(16)] + [dcol(True)], None, [chain, ColumnExpression("c", 16, D)], "17 nullable inputs")
        fp(sixteen[:15] + [scol(d1), scol(d2)], fe(Fn.CMP_LT, ColumnExpression("s", 15, S), ColumnExpression("t", 16, S)),
           [ColumnExpression("c", i, D) for i in range(14)], "too many columns + aux tables")
    ctx.close()
    with open(os.path.join(out, name, "errors.txt"), "w") as f:
        f.write("".join(e + "\n" for e in errors))


def run_driver(repo, out):
    csrc = os.path.join(repo, "queryengine_amd", "csrc")
    cases = os.path.join(out, "cases")
    os.makedirs(cases, exist_ok=True)
    exe = os.path.join(out, "dump_codegen_cases")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{csrc}",
                           os.path.join(HERE, "dump_codegen_cases.cpp"), "-o", exe, f"-L{csrc}", "-lqe_hip",
                           f"-Wl,-rpath,{csrc}", f"-Wl,-rpath,{rocm}/lib"])
    subprocess.check_call([exe, cases])
    os.remove(exe)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    ap.add_argument("--repo", default=os.path.dirname(HERE), help="checkout to load queryengine_amd and libqe_hip.so from")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--seed", help="an earlier output directory: start from copies of its JIT caches")
    ap.add_argument("--only", help="comma-separated option-set names")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    repo, out = os.path.abspath(args.repo), os.path.abspath(args.out)
    sets = [s for s in option_sets() if not args.only or s[0] in args.only.split(",")]
    if args.child:
        name, tuning, cmp, scope = next(s for s in sets if s[0] == args.child)
        run_option_set(repo, out, name, tuning, cmp, scope)
        return
    os.makedirs(out, exist_ok=True)
    for name, *_ in sets:
        if args.seed and os.path.isdir(os.path.join(args.seed, name)):
            shutil.copytree(os.path.join(args.seed, name), os.path.join(out, name), dirs_exist_ok=True)
        os.makedirs(os.path.join(out, name), exist_ok=True)
    run_driver(repo, out)
    pending, running, failed = list(sets), [], []
    while pending or running:
        while pending and len(running) < max(1, args.jobs):
            name = pending.pop(0)[0]
            cmd = [sys.executable, os.path.abspath(__file__), "--out", out, "--repo", repo, "--child", name]
            running.append((name, subprocess.Popen(cmd)))
        name, proc = running.pop(0)
        if proc.wait() != 0:
            failed.append(name)
    with open(os.path.join(out, "errors.txt"), "w") as f:
        for name, *_ in sets:
            path = os.path.join(out, name, "errors.txt")
            if os.path.exists(path):
                f.write(open(path).read())
                os.remove(path)
    if failed:
        sys.exit("option sets that did not finish: " + ", ".join(failed))


if __name__ == "__main__":
    main()
