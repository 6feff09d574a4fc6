#!/usr/bin/env python3
"""Ordered-set aggregates per group on the device: a result of --rows rows (INT64 key, DOUBLE value), generated on the device
with qe_batch_generate and an identity projection, goes through qe_result_group_ordered grouped by the key, for several group
counts: MEDIAN alone, and COUNT_DISTINCT + PERCENTILE_DISC + MODE + MEDIAN on the one value column (one sort).  The same run
times qe_result_order_by_keys on the same (key, value) keys -- the sort, with its gather of every column, is the floor the
call adds to -- and qe_stream_read_bandwidth.  Every call runs --warmup times unmeasured, then --reps times; the best
synchronised wall time around the ABI call is reported (the calls return after their own stream synchronisation).  The
quantity to report is (call - sort), next to the time a plain read stream of this run needs for the bytes DESIGN.md 3.10 models
for the passes behind the sort.  The 1-group MODE case -- every run of the input raises the same entry, the worst case of the
integer max -- is printed on a line of its own.

    python tools/bench_ordered.py [--rows 100000000] [--groups 1,1000,10000000] [--reps 5] [--warmup 1] [--out profiles/ordered_agg_summary.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from queryengine_amd import ColumnExpression, DataType  # noqa: E402
from queryengine_amd import engine as E  # noqa: E402
from queryengine_amd import native as N  # noqa: E402

# DESIGN.md 3.10, bytes behind the sort.  Per row: the boundary flags (row id, two key values, two bits written), word ranks of
# pstart (bitmap twice, a u32 per word) and its compaction; all four add the ranks and the compaction of peer.  Per group: the
# group start, the bisection's result, the key's row list and gather, and per function its reads through the row ids and its
# output.  Per run of equal values (MODE): the compacted start written, read twice, the group lookup and the group's bounds.
ROW_BYTES = {"median": 20.25 + 0.3125 + 0.125, "all four": 20.25 + 2 * (0.3125 + 0.125)}
GROUP_BYTES = {"median": 4 + 12 + 12 + 20 + 44.125, "all four": 4 + 12 + 12 + 20 + 44.125 + 52 + 40.25 + 44.25}
RUN_BYTES = {"median": 0.0, "all four": 4 + 8 + 28}


def spec(kind, col_id, modulus=0):
    s = N.GenSpec()
    s.kind, s.col_id, s.modulus = kind, col_id, modulus
    return s


def best_ms(ctx, call, reps, warmup):
    times = []
    for i in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            times.append(dt)
        out.free()
    return min(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--groups", default="1,1000,10000000")
    ap.add_argument("--values", type=int, default=1000, help="distinct values of the DOUBLE column (runs per group for MODE)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    n = a.rows
    ctx = E.Context(device=0)
    gbps = ctx.stream_read_bandwidth(1 << 30, 5)
    lines = [f"ordered-set aggregates per group on one device: {n} rows (INT64 key, DOUBLE value of {a.values} distinct values); best of {a.reps}, "
             f"{a.warmup} warm-up run(s) excluded; synchronised wall time around the call",
             f"qe_stream_read_bandwidth of this run: {gbps:.0f} GB/s",
             f"{'groups':>9} {'function':>9} {'call ms':>9} {'sort ms':>9} {'call - sort':>11} {'model MB':>9} {'as stream ms':>12} {'/ stream':>9} | "
             f"{'counted groups':>14} {'sorts':>5} {'radix passes':>12}"]
    projs = [ctx.compile(ColumnExpression("k", 0, DataType.INT64)), ctx.compile(ColumnExpression("v", 1, DataType.DOUBLE))]
    sets = {"median": [E.MEDIAN(1)], "all four": [(N.OSA_COUNT_DISTINCT, 1), (N.OSA_PERCENTILE_DISC, 1, 0.5), (N.OSA_MODE, 1), E.MEDIAN(1)]}
    mode_line = None
    for groups in [int(v) for v in a.groups.split(",")]:
        batch = E.DeviceBatch.generate(ctx, [spec(N.GEN_I64_MOD, 0, groups), spec(N.GEN_F64_MOD, 1, a.values)], n, seed=13)
        res = E.filter_project(ctx, batch, None, projs)
        sort_ms = best_ms(ctx, lambda: ctx.order_by_keys(res, [(0, False), (1, False)]), a.reps, a.warmup)
        for name, fns in sets.items():
            ms = best_ms(ctx, lambda: ctx.group_ordered(res, [0], fns), a.reps, a.warmup)
            st = ctx.last_ordered_stats()
            runs = min(n, st["groups"] * a.values)
            model = ROW_BYTES[name] * n + GROUP_BYTES[name] * st["groups"] + RUN_BYTES[name] * runs
            stream_ms = model / (gbps * 1e9) * 1e3
            lines.append(f"{groups:>9} {name:>9} {ms:>9.3f} {sort_ms:>9.3f} {ms - sort_ms:>11.3f} {model / 1e6:>9.0f} {stream_ms:>12.3f} "
                         f"{(ms - sort_ms) / stream_ms:>8.1f}x | {st['groups']:>14} {st['sorts']:>5} {st['radix_passes']:>12}")
        if groups == 1:
            ms = best_ms(ctx, lambda: ctx.group_ordered(res, [0], [(N.OSA_MODE, 1)]), a.reps, a.warmup)
            mode_line = f"MODE alone over 1 group ({a.values} runs, every one raising the same entry): {ms:.3f} ms, call - sort {ms - sort_ms:.3f} ms"
        res.free(); batch.free()
    if mode_line:
        lines.append(mode_line)
    ctx.close()
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
