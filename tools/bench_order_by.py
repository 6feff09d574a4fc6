#!/usr/bin/env python3
"""ORDER BY on the device: the full sort (qe_result_order_by, qe_result_order_by_keys) against ORDER BY .. LIMIT k (the
top-k selection), on one result of --rows rows: a DOUBLE key uniform in [0, 1), a coarse INT32 column (16 values) and an
INT64 payload.  Every case runs --warmup times unmeasured, then --reps times; the best synchronised wall time around the
ABI call is reported (the call returns after its own stream synchronisation), with the speed-up over the full single-key
sort of the same run and what qe_ctx_last_sort_stats says the call did.

    python tools/bench_order_by.py [--rows 100000000] [--reps 5] [--warmup 1] [--json out.json] [--single-key-only]

--single-key-only measures qe_result_order_by alone (the one call older builds of the library have too)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from queryengine_amd import Column, ColumnExpression, DataType  # noqa: E402
from queryengine_amd import engine as E  # noqa: E402

D, I64, I32 = DataType.DOUBLE, DataType.INT64, DataType.INT32


def best_ms(ctx, call, reps, warmup):
    times = []
    for i in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        res = call()
        dt = (time.perf_counter() - t0) * 1e3
        res.free()
        if i >= warmup:
            times.append(dt)
    return min(times), sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=None)
    ap.add_argument("--single-key-only", action="store_true")
    a = ap.parse_args()

    n = a.rows
    rng = np.random.default_rng(2024)
    cols = [Column(D, rng.random(n)), Column(I32, rng.integers(0, 16, n).astype(np.int32)), Column(I64, np.arange(n, dtype=np.int64))]
    ctx = E.Context(device=0)
    batch = E.DeviceBatch.from_columns(ctx, cols)
    res = E.filter_project(ctx, batch, None, [ctx.compile(ColumnExpression(f"c{i}", i, c.type)) for i, c in enumerate(cols)])
    batch.free()
    del cols

    cases = [("qe_result_order_by (1 key ASC)", lambda: ctx.order_by(res, 0))]
    if not a.single_key_only:
        cases += [("order_by_keys, 1 key ASC, no limit", lambda: ctx.order_by_keys(res, [(0, False)])),
                  ("order_by_keys, 1 key DESC, no limit", lambda: ctx.order_by_keys(res, [(0, True)])),
                  ("order_by_keys, 2 keys (INT32 coarse, DOUBLE)", lambda: ctx.order_by_keys(res, [(1, False), (0, False)]))]
        for k in (100, 1_000_000):
            for desc in (False, True):
                cases.append((f"top-k, k = {k}, {'DESC' if desc else 'ASC'}",
                              lambda k=k, desc=desc: ctx.order_by_keys(res, [(0, desc)], min(k, n))))
        cases.append(("top-k, k = 100, 2 keys (DOUBLE DESC, INT32)", lambda: ctx.order_by_keys(res, [(0, True), (1, False)], min(100, n))))

    out = {"rows": n, "reps": a.reps, "warmup": a.warmup, "cases": []}
    print(f"ORDER BY on one device, {n} rows (DOUBLE key uniform in [0, 1), INT32 coarse, INT64 payload); best of {a.reps}, "
          f"{a.warmup} warm-up run(s) excluded; synchronised wall time around the call")
    print(f"{'case':<48} {'best ms':>10} {'median ms':>10} {'vs full sort':>13}  what the call did")
    full = None
    for name, call in cases:
        best, med = best_ms(ctx, call, a.reps, a.warmup)
        stats = {} if a.single_key_only else ctx.last_sort_stats()
        if full is None:
            full = best
        ratio = full / best
        out["cases"].append({"case": name, "best_ms": best, "median_ms": med, "speedup_vs_full_sort": ratio, "stats": stats})
        what = (f"{stats['path']}: {stats['sorted_rows']} rows sorted, {stats['radix_passes']} radix passes, "
                f"{stats['select_passes']} selection passes") if stats else ""
        print(f"{name:<48} {best:>10.3f} {med:>10.3f} {ratio:>12.2f}x  {what}")
    res.free()
    ctx.close()
    status = 0
    if not a.single_key_only:
        # the floor the top-k selection has to meet: k = 100 at least 3x faster than the full single-key sort of this run
        worst = min(c["speedup_vs_full_sort"] for c in out["cases"] if c["case"] in ("top-k, k = 100, ASC", "top-k, k = 100, DESC"))
        out["topk_100_floor"] = {"required": 3.0, "measured": worst, "met": worst >= 3.0}
        print(f"top-k at k = 100 against the full single-key sort: {worst:.2f}x (floor 3x): {'PASS' if worst >= 3.0 else 'FAIL'}")
        status = 0 if worst >= 3.0 else 1
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return status


if __name__ == "__main__":
    sys.exit(main())
