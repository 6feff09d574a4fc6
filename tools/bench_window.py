#!/usr/bin/env python3
"""Window functions on the device: a result of --rows rows (INT64 partition key, DOUBLE order key, DOUBLE value), generated on
the device with qe_batch_generate and an identity projection, goes through qe_result_window with ROW_NUMBER, a running SUM
of the value and LAG(value, 1), partitioned by the key and ordered by the order key, for several partition counts.  The
same run times qe_result_order_by_keys on the same two keys: the sort (and the gather of every column) is the floor the
window adds to.  Every call runs --warmup times unmeasured, then --reps times; the best synchronised wall time around the
ABI call is reported (the calls return after their own stream synchronisation).  (window - sort) is set against the time a
plain read stream of this run (qe_stream_read_bandwidth) needs for the bytes the scan passes read and write by the model of
DESIGN.md 3.9.  The same run, on the same keys, then times a SUM of the value alone three ways -- the running frame
(qe_result_window), ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING, and the whole partition (both qe_result_window_frames) -- so that
(framed - running) stands next to the bytes the frame passes add by the model.

    python tools/bench_window.py [--rows 100000000] [--partitions 1,1000,10000000] [--reps 3] [--warmup 1] [--json out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from queryengine_amd import ColumnExpression, DataType  # noqa: E402
from queryengine_amd import engine as E  # noqa: E402
from queryengine_amd import native as N  # noqa: E402

# bytes per row the passes behind the sort read + write: boundary flags over two keys (row id, two key
# values; two bits written), the partition-start index (bitmap twice, 4 written), ROW_NUMBER (4 read, 8 written), the
# running SUM (value twice, 8 written, bitmaps), LAG (two start indices, value, 8 written, a validity bit)
# what a framed SUM adds to the running one: the start and end index scans (bitmap twice, 4 written, each), per
# pair scan the value twice + bitmaps + a {f64, u32} pair written, and the combine (two indices, the pairs read, 8 written + a
# bit); minus the running scan it replaces.  A bounded frame keeps two pair scans, a whole-partition frame one.
PAIR_SCAN, RUNNING_SCAN, INDEX_SCANS = 8 + 8 + 0.5 + 12, 8 + 8 + 8 + 0.5, 2 * (0.25 + 4)
FRAME_MODEL_BYTES_PER_ROW = {"sliding (3, 3)": INDEX_SCANS + 2 * PAIR_SCAN + (4 + 4 + 24 + 8 + 0.125) - RUNNING_SCAN,
                             "whole partition": INDEX_SCANS + PAIR_SCAN + (4 + 4 + 12 + 8 + 0.125) - RUNNING_SCAN}
MODEL_BYTES_PER_ROW = {"flags": 4 + 2 * 8 + 0.25, "start index": 0.25 + 4, "ROW_NUMBER": 4 + 8, "SUM": 8 + 8 + 8 + 0.5, "LAG": 4 + 4 + 8 + 8 + 0.125}


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
    ap.add_argument("--partitions", default="1,1000,10000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.rows
    ctx = E.Context(device=0)
    gbps = ctx.stream_read_bandwidth(1 << 30, 5)
    model_bytes = sum(MODEL_BYTES_PER_ROW.values()) * n
    stream_ms = model_bytes / (gbps * 1e9) * 1e3
    out = {"rows": n, "reps": a.reps, "warmup": a.warmup, "stream_read_gbps": gbps, "model_bytes_per_row": MODEL_BYTES_PER_ROW,
           "scan_bytes_as_stream_ms": stream_ms, "frame_model_bytes_per_row": FRAME_MODEL_BYTES_PER_ROW, "cases": [], "frame_cases": []}
    frame_lines = []
    print(f"window functions on one device: {n} rows (INT64 partition key, DOUBLE order key, DOUBLE value); ROW_NUMBER, running SUM, LAG 1; "
          f"best of {a.reps}, {a.warmup} warm-up run(s) excluded; synchronised wall time around the call")
    print(f"qe_stream_read_bandwidth of this run: {gbps:.0f} GB/s; the scan passes' modelled {model_bytes / 1e6:.0f} MB as a stream: {stream_ms:.3f} ms")
    print(f"{'partitions':>11} {'window ms':>10} {'sort ms':>9} {'window - sort':>13} {'/ stream':>9} | {'counted partitions':>18} {'tiles':>8} {'trips':>6}")
    projs = [ctx.compile(ColumnExpression("p", 0, DataType.INT64)), ctx.compile(ColumnExpression("o", 1, DataType.DOUBLE)),
             ctx.compile(ColumnExpression("v", 2, DataType.DOUBLE))]
    fns = [(N.WIN_ROW_NUMBER,), (N.WIN_SUM, 2), (N.WIN_LAG, 2, 1)]
    for nparts in [int(v) for v in a.partitions.split(",")]:
        batch = E.DeviceBatch.generate(ctx, [spec(N.GEN_I64_MOD, 0, nparts), spec(N.GEN_F64_UNIT, 1), spec(N.GEN_F64_UNIT, 2)], n, seed=13)
        res = E.filter_project(ctx, batch, None, projs)
        sort_ms = best_ms(ctx, lambda: ctx.order_by_keys(res, [(0, False), (1, False)]), a.reps, a.warmup)
        window_ms = best_ms(ctx, lambda: ctx.window(res, [0], [(1, False)], fns), a.reps, a.warmup)
        st = ctx.last_window_stats()
        ratio = (window_ms - sort_ms) / stream_ms
        out["cases"].append({"partitions": nparts, "window_ms": window_ms, "sort_ms": sort_ms, "scan_over_stream": ratio, "stats": st})
        print(f"{nparts:>11} {window_ms:>10.3f} {sort_ms:>9.3f} {window_ms - sort_ms:>13.3f} {ratio:>8.1f}x | {st['partitions']:>18} {st['tiles']:>8} {st['trips']:>6}")
        # the same keys, one SUM: running / sliding / whole partition
        U = N.FRAME_UNBOUNDED
        running_ms = best_ms(ctx, lambda: ctx.window(res, [0], [(1, False)], [(N.WIN_SUM, 2)]), a.reps, a.warmup)
        fc = {"partitions": nparts, "sort_ms": sort_ms, "running_sum_ms": running_ms}
        line = f"{nparts:>11} {sort_ms:>9.3f} {running_ms:>11.3f}"
        for name, frame in (("sliding (3, 3)", (3, 3)), ("whole partition", (U, U))):
            ms = best_ms(ctx, lambda: ctx.window(res, [0], [(1, False)], [(N.WIN_SUM, 2, 0) + frame]), a.reps, a.warmup)
            model_ms = FRAME_MODEL_BYTES_PER_ROW[name] * n / (gbps * 1e9) * 1e3
            fc[name] = {"ms": ms, "framed_minus_running_ms": ms - running_ms, "model_stream_ms": model_ms}
            line += f" | {ms:>10.3f} {ms - running_ms:>9.3f} {model_ms:>9.3f}"
        out["frame_cases"].append(fc)
        frame_lines.append(line)
        res.free(); batch.free()
    print(f"a SUM of the value alone on the same keys: running frame (qe_result_window) against ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING and the whole "
          f"partition (qe_result_window_frames); modelled extra bytes per row: " + ", ".join(f"{k} {v:.1f}" for k, v in FRAME_MODEL_BYTES_PER_ROW.items()))
    print(f"{'partitions':>11} {'sort ms':>9} {'running ms':>11} | {'sliding ms':>10} {'- running':>9} {'model ms':>9} | {'whole ms':>10} {'- running':>9} {'model ms':>9}")
    for line in frame_lines:
        print(line)
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
