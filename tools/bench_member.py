#!/usr/bin/env python3
"""What a set-membership predicate costs in a filter, route by route; one process, executions alternating between the plans.

On the cfg 2 batch (a INT64 uniform in [0, 1000), b INT64, c DOUBLE), SELECT a + b WHERE .. with, for m = 2, 4, 8, 16, 32:

  floor   a < m                               the plain comparison at the same selectivity (m / 1000)
  chain   a IN (m values)                     inline compare chain           (QE_IN_CHAIN_UPTO=32 while the plan is built)
  bits    a IN (m values)                     bit table over a - min         (QE_IN_CHAIN_UPTO=0)
  hash    a IN (m values)                     hash set of 64-bit images      (QE_IN_CHAIN_UPTO=0 QE_IN_BITS_SPAN=1)
  or      a = v1 OR .. OR a = vm              what had to be written before

and the hash set at m = 256, 4096 and 65 536 literals, of which 256 lie in the column's range (floor: a < 256).  The variants
of one m use different values of the same count, so that each is a plan of its own.  The two switches are read when a plan
is built, never afterwards.

On the cfg 4 batch (s STRING over 1000 keys, v DOUBLE), SELECT s, v WHERE ..: the dictionary equality plan s = 'k0042', s IN
(3 keys), s IN (40 keys), s LIKE 'k004%' (10 codes) and s LIKE 'k00%' (100 codes).

Per plan: rows out, kernel ms (median and min of --reps executions).  One GPU."""
import argparse
import contextlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from queryengine_amd import (ColumnExpression, DataType, Function, FunctionExpression, NumericLiteralExpression,
                             SetFunction, StringLiteralExpression)
from queryengine_amd import engine as E
from queryengine_amd import workloads as W

D, I64, B, S = DataType.DOUBLE, DataType.INT64, DataType.BOOLEAN, DataType.STRING
Fn = Function
SetFn = SetFunction
num, lit = NumericLiteralExpression, StringLiteralExpression


def fn(f, t, *ops):
    return FunctionExpression(f, list(ops), t)


def in_(x, values):
    mk = lit if isinstance(values[0], str) else (lambda v: num(float(v)))
    return fn(SetFn.IN, B, x, *[mk(v) for v in values])


def spread(m, phase):
    """m distinct values of [0, 1000), spread over the whole range; another `phase` gives another set."""
    return sorted({(phase + (k * 1000) // m) % 1000 for k in range(m)})


def cfg2_plans():
    a, b = ColumnExpression("a", 0, I64), ColumnExpression("b", 1, I64)
    out = [fn(Fn.ADD, I64, a, b)]
    plans = []   # (name, environment while the plan is built, filter, projections)
    for m in (2, 4, 8, 16, 32):
        plans.append((f"m={m:<5} floor  a < {m}", {}, fn(Fn.CMP_LT, B, a, num(float(m))), out))
        plans.append((f"m={m:<5} chain", {"QE_IN_CHAIN_UPTO": "32"}, in_(a, spread(m, 1)), out))
        plans.append((f"m={m:<5} bits", {"QE_IN_CHAIN_UPTO": "0"}, in_(a, spread(m, 2)), out))
        plans.append((f"m={m:<5} hash", {"QE_IN_CHAIN_UPTO": "0", "QE_IN_BITS_SPAN": "1"}, in_(a, spread(m, 3)), out))
        chain = None
        for v in spread(m, 4):
            eq = fn(Fn.CMP_EQ, B, a, num(float(v)))
            chain = eq if chain is None else fn(Fn.OR, B, chain, eq)
        plans.append((f"m={m:<5} or     a = v1 OR ..", {}, chain, out))
    plans.append(("m=256   floor  a < 256", {}, fn(Fn.CMP_LT, B, a, num(256.0)), out))
    for m in (256, 4096, 65536):
        values = spread(256, 5 + m % 7) + [1000 + 7919 * k for k in range(m - 256)]   # the rest lies outside the column's range
        plans.append((f"m={m:<5} hash", {"QE_IN_CHAIN_UPTO": "0", "QE_IN_BITS_SPAN": "1"}, in_(a, values), out))
    plans.append(("m=256   bits", {"QE_IN_CHAIN_UPTO": "0"}, in_(a, spread(256, 3)), out))
    return plans


def cfg4_plans():
    s, v = ColumnExpression("s", 0, S), ColumnExpression("v", 1, D)
    out = [s, v]
    keys = ["k%04d" % i for i in range(1000)]
    return [("s = 'k0042'", {}, fn(Fn.CMP_EQ, B, s, lit("k0042")), out),
            ("s IN (3 keys)", {}, in_(s, [keys[42], keys[500], keys[999]]), out),
            ("s IN (40 keys)", {}, in_(s, keys[100:140]), out),
            ("s LIKE 'k004%' (10 codes)", {}, fn(SetFn.LIKE, B, s, lit("k004%")), out),
            ("s LIKE 'k00%' (100 codes)", {}, fn(SetFn.LIKE, B, s, lit("k00%")), out)]


@contextlib.contextmanager
def switches(env):
    """The plan's switches for as long as it may be built: a plan is built again for every geometry it tries."""
    saved = {k: os.environ.get(k) for k in ("QE_IN_CHAIN_UPTO", "QE_IN_BITS_SPAN")}
    for k in saved:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def measure(ctx, batch, plans, warmup, reps):
    compiled = []
    for name, env, flt, projs in plans:
        with switches(env):
            cf, cp = ctx.compile(flt), [ctx.compile(p) for p in projs]
            E.prepare(ctx, batch, cf, cp)
        compiled.append((name, env, cf, cp, []))
    nout = {}
    for rep in range(warmup + reps):
        for name, env, cf, cp, ts in compiled:
            with switches(env):
                r = E.filter_project(ctx, batch, cf, cp)
            nout[name] = r.count
            r.free()
            if rep >= warmup:
                ts.append(ctx.kernel_time()[0])
    lines = [f"{'plan':<34} {'rows out':>12} {'kernel ms (median / min)':>26}"]
    for name, env, cf, cp, ts in compiled:
        ts.sort()
        lines.append(f"{name:<34} {nout[name]:>12} {ts[len(ts) // 2]:>17.3f} / {ts[0]:<6.3f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=4, help="executions per plan before the timed ones (the plan measures its conjuncts and picks its geometry)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    ctx = E.Context(device=0, profile=True)
    lines = [f"{args.rows} rows; {args.reps} timed executions per plan, alternating, after {args.warmup} warm-up rounds", "",
             "cfg 2 batch: SELECT a + b WHERE <predicate on a>"]
    wl = W.config2(args.rows)
    batch = E.DeviceBatch.generate(ctx, [c.spec(ctx) for c in wl.columns], args.rows)
    lines += measure(ctx, batch, cfg2_plans(), args.warmup, args.reps)
    batch.free()
    print("\n".join(lines), flush=True)
    wl = W.config4(args.rows)
    batch = E.DeviceBatch.generate(ctx, [c.spec(ctx) for c in wl.columns], args.rows)
    tail = ["", "cfg 4 batch: SELECT s, v WHERE <predicate on s>"] + measure(ctx, batch, cfg4_plans(), args.warmup, args.reps)
    print("\n".join(tail), flush=True)
    lines += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    batch.free()
    ctx.close()


if __name__ == "__main__":
    main()
