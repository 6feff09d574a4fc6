#!/usr/bin/env python3
"""What IS_NOT_NULL and COALESCE cost in a filter: three plans on the cfg 2 batch with ~1 % NULLs in every input
(a, b INT64, c DOUBLE, each with a validity bitmap), one process, executions alternating between the plans.

  (i)   a < 100 AND c < 0.5                   SELECT a + b      the plan that could be written before
  (ii)  IS_NOT_NULL(c) AND a < 100            SELECT a + b      c is read through its validity bitmap alone
  (iii) COALESCE(c, 0.0) < 0.5 AND a < 100    SELECT a + b

Per plan: kernel ms (median and min of --reps executions), the algorithmic bytes computed from the shapes -- every input
column of the plan in full (8 bytes per row, + 1 bit per row for its validity bitmap; for (ii) c counts as its bitmap alone:
rows / 8 bytes) plus the output rows (8 bytes + 1 validity bit each) -- and the fraction of the 8 TB/s HBM peak, as bench.py
reports it.  One GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from queryengine_amd import ColumnExpression, DataType, Function, FunctionExpression, NumericLiteralExpression
from queryengine_amd import engine as E
from queryengine_amd import workloads as W

HBM_PEAK_GBPS = 8000.0
D, I64, B = DataType.DOUBLE, DataType.INT64, DataType.BOOLEAN
Fn = Function


def plans():
    a, b, c = ColumnExpression("a", 0, I64), ColumnExpression("b", 1, I64), ColumnExpression("c", 2, D)
    num = NumericLiteralExpression

    def fn(f, t, *ops):
        return FunctionExpression(f, list(ops), t)
    a_lt = fn(Fn.CMP_LT, B, a, num(100.0))
    out = [fn(Fn.ADD, I64, a, b)]
    # (name, filter, projections, bytes read per row: 8-byte columns in full + validity bits)
    return [("(i)   a < 100 AND c < 0.5", fn(Fn.AND, B, a_lt, fn(Fn.CMP_LT, B, c, num(0.5))), out, 3 * 8 + 3 / 8),
            ("(ii)  IS_NOT_NULL(c) AND a < 100", fn(Fn.AND, B, fn(Fn.IS_NOT_NULL, B, c), a_lt), out, 2 * 8 + 3 / 8),
            ("(iii) COALESCE(c, 0.0) < 0.5 AND a < 100",
             fn(Fn.AND, B, fn(Fn.CMP_LT, B, fn(Fn.COALESCE, D, c, num(0.0)), num(0.5)), a_lt), out, 3 * 8 + 3 / 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=4, help="executions per plan before the timed ones (the plan measures its conjuncts and picks its geometry)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    ctx = E.Context(device=0, profile=True)
    wl = W.config2(args.rows, null_pct=1)
    batch = E.DeviceBatch.generate(ctx, [c.spec(ctx) for c in wl.columns], args.rows)
    compiled = []
    for name, flt, projs, read_b in plans():
        cf, cp = ctx.compile(flt), [ctx.compile(p) for p in projs]
        E.prepare(ctx, batch, cf, cp)
        compiled.append((name, cf, cp, read_b, []))
    nout = {}
    for rep in range(args.warmup + args.reps):           # alternating: plan (i), (ii), (iii), (i), ..
        for name, cf, cp, read_b, ts in compiled:
            r = E.filter_project(ctx, batch, cf, cp)
            nout[name] = r.count
            r.free()
            if rep >= args.warmup:
                ts.append(ctx.kernel_time()[0])
    lines = [f"cfg 2 batch, {args.rows} rows, 1 % NULLs per input column; {args.reps} timed executions per plan, alternating, after {args.warmup} warm-up rounds",
             f"{'plan':<44} {'rows out':>12} {'kernel ms (median / min)':>26} {'algorithmic GB':>15} {'GB/s':>8} {'of 8 TB/s':>10}"]
    for name, cf, cp, read_b, ts in compiled:
        ts.sort()
        med, mn = ts[len(ts) // 2], ts[0]
        alg = args.rows * read_b + nout[name] * (8 + 1 / 8)
        gbps = alg / (med * 1e-3) / 1e9
        lines.append(f"{name:<44} {nout[name]:>12} {med:>17.3f} / {mn:<6.3f} {alg / 1e9:>15.3f} {gbps:>8.0f} {gbps / HBM_PEAK_GBPS:>10.3f}")
    report = "\n".join(lines)
    print(report, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(report + "\n")
    batch.free()
    ctx.close()


if __name__ == "__main__":
    main()
