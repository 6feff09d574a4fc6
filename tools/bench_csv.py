#!/usr/bin/env python3
"""CSV text -> device batch: the host parser (qe_csv_parse + qe_csv_pin) against the device parser (qe_csv_parse_device),
on a tripdata-shaped text synthesised in memory (the 18 fields and header of the NYC yellow taxi file of 2019-01, ~93 bytes
per record), and the two queries of the reference's Tripdata.kt end to end, from the bytes to the rows on the host.

    python tools/bench_csv.py [--rows 7700000] [--reps 3] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from queryengine_amd import DataType, Field, Schema  # noqa: E402

HEADER = ["VendorID", "tpep_pickup_datetime", "tpep_dropoff_datetime", "passenger_count", "trip_distance", "RatecodeID",
          "store_and_fwd_flag", "PULocationID", "DOLocationID", "payment_type", "fare_amount", "extra", "mta_tax", "tip_amount",
          "tolls_amount", "improvement_surcharge", "total_amount", "congestion_surcharge"]
_STRINGS = {"tpep_pickup_datetime", "tpep_dropoff_datetime", "store_and_fwd_flag"}
SCHEMA = Schema([Field(h, DataType.STRING if h in _STRINGS else DataType.DOUBLE) for h in HEADER])
PROJECTION = ["tip_amount", "fare_amount", "passenger_count"]          # Tripdata.kt:9-12
QUERIES = ["SELECT MIN(tip_amount), MAX(tip_amount) FROM tripdata",
           "SELECT passenger_count, MIN(fare_amount), MAX(fare_amount) FROM tripdata"]


def _record(rng):
    t0 = rng.randrange(31 * 86400)
    t1 = t0 + rng.randrange(60, 3600)
    ts = lambda t: f"2019-01-{1 + t // 86400:02d} {t // 3600 % 24:02d}:{t // 60 % 60:02d}:{t % 60:02d}"
    fare = rng.randrange(250, 8000) / 100 if rng.random() < 0.9 else rng.choice([2.5, 52, 0, -52])
    tip = round(fare * rng.choice([0, 0, 0.1, 0.15, 0.2, 0.25]), 2)
    total = round(fare + 0.5 + 0.5 + 0.3 + tip, 2)
    f = lambda v: f"{v:g}" if rng.random() < 0.5 else f"{v}"
    return ",".join([str(rng.choice([1, 2])), ts(t0), ts(t1), str(rng.choice([1, 1, 1, 1, 2, 3, 5, 6, 0])),
                     f"{rng.randrange(0, 3000) / 100:.2f}", str(rng.choice([1, 1, 1, 2, 5])), rng.choice("NNNNNNNNY"),
                     str(rng.randrange(1, 266)), str(rng.randrange(1, 266)), str(rng.choice([1, 1, 2, 3])), f(fare), "0.5",
                     "0.5", f(tip), "0", "0.3", f(total), ""])


def synthesize(nrows, seed=2019, pool=1 << 16):
    """nrows tripdata-shaped records (drawn from `pool` distinct ones) behind the 2019-01 header, as bytes."""
    rng = random.Random(seed)
    recs = [(_record(rng) + "\n").encode() for _ in range(min(pool, max(nrows, 1)))]
    pick = [rng.randrange(len(recs)) for _ in range(nrows)]
    return (",".join(HEADER) + "\n").encode() + b"".join([recs[i] for i in pick])


def _names(fields):
    return ((C.c_char_p * len(fields))(*[f.name.encode() for f in fields]), (C.c_int32 * len(fields))(*[int(f.type) for f in fields]))


def host_parse_pin(ctx, text, fields):
    lib = ctx._lib
    names, types = _names(fields)
    t, b = C.c_void_p(), C.c_void_p()
    t0 = time.perf_counter()
    st = lib.qe_csv_parse(ctx.handle, text, len(text), len(fields), names, types, C.byref(t))
    t1 = time.perf_counter()
    st = st or lib.qe_csv_pin(ctx.handle, t, C.byref(b))
    t2 = time.perf_counter()
    assert st == 0, lib.qe_last_error(ctx.handle)
    lib.qe_csv_free(ctx.handle, t)
    lib.qe_batch_free(ctx.handle, b)
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


def device_parse(ctx, text, fields):
    from queryengine_amd import native as N
    lib = ctx._lib
    names, types = _names(fields)
    b = C.c_void_p()
    t0 = time.perf_counter()
    st = lib.qe_csv_parse_device(ctx.handle, text, len(text), len(fields), names, types, C.byref(b))
    wall = (time.perf_counter() - t0) * 1e3
    assert st == 0, lib.qe_last_error(ctx.handle)
    s = N.CsvDeviceStats()
    lib.qe_csv_device_last_stats(ctx.handle, C.byref(s))
    lib.qe_batch_free(ctx.handle, b)
    return wall, s


def pure_h2d_ms(nbytes, reps):
    import torch
    src = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src, non_blocking=True)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=7_700_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--all-fields", action="store_true", help="project all 18 fields instead of Tripdata.kt's three")
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    from queryengine_amd import engine as E
    from queryengine_amd.csv_table import DeviceCsvTable, read_csv_native
    from queryengine_amd.planner import Mode, query
    from queryengine_amd.table import ColumnarTable

    t0 = time.perf_counter()
    text = synthesize(a.rows)
    gb = len(text) / 1e9
    print(f"text: {a.rows} rows, {len(text) / 1e6:.1f} MB ({(time.perf_counter() - t0):.1f} s to synthesise)", flush=True)
    fields = SCHEMA.fields if a.all_fields else [SCHEMA[n] for n in PROJECTION]
    ctx = E.Context(device=0)
    out = {"rows": a.rows, "bytes": len(text), "fields": len(fields)}
    dev = [device_parse(ctx, text, fields) for _ in range(a.reps + 1)][1:]   # the first call warms the pools
    assert all(s.host_fallback == 0 and s.host_patched_fields == 0 and s.nrows == a.rows for _, s in dev)
    med = lambda xs: statistics.median(xs)
    out["device_wall_ms"] = med([w for w, _ in dev])
    out["device_h2d_ms"] = med([s.h2d_ms for _, s in dev])
    out["device_kernel_ms"] = med([s.kernel_ms for _, s in dev])
    out["pure_h2d_ms"] = pure_h2d_ms(len(text), a.reps)
    print(f"device: {out['device_wall_ms']:.1f} ms wall ({gb / out['device_wall_ms'] * 1e3:.1f} GB/s): h2d {out['device_h2d_ms']:.1f} ms, "
          f"kernels {out['device_kernel_ms']:.1f} ms ({gb / out['device_kernel_ms'] * 1e3:.1f} GB/s); pure pinned H2D of the text "
          f"{out['pure_h2d_ms']:.1f} ms", flush=True)
    if not a.skip_host:
        host = [host_parse_pin(ctx, text, fields) for _ in range(max(1, a.reps - 1))]
        out["host_parse_ms"] = med([p for p, _ in host])
        out["host_pin_ms"] = med([q for _, q in host])
        hw = out["host_parse_ms"] + out["host_pin_ms"]
        print(f"host: parse {out['host_parse_ms']:.1f} ms ({gb / out['host_parse_ms'] * 1e3:.2f} GB/s) + pin {out['host_pin_ms']:.1f} ms; "
              f"device path {hw / out['device_wall_ms']:.1f}x faster", flush=True)
    # Tripdata.kt's two queries, bytes -> rows on the host
    sch = Schema([SCHEMA[n] for n in PROJECTION])
    for i, sql in enumerate(QUERIES):
        t0 = time.perf_counter()
        rows_d = query("tripdata", sql, Mode.GPU_FUSED, table=DeviceCsvTable(text, sch), ctx=ctx)
        out[f"q{i + 1}_device_ms"] = (time.perf_counter() - t0) * 1e3
        line = f"Q{i + 1} {sql}: device path {out[f'q{i + 1}_device_ms']:.1f} ms"
        if not a.skip_host:
            t0 = time.perf_counter()
            t = read_csv_native(ctx, text, sch)
            rows_h = query("tripdata", sql, Mode.GPU_FUSED, table=ColumnarTable(t.schema, t.columns), ctx=ctx)
            out[f"q{i + 1}_host_ms"] = (time.perf_counter() - t0) * 1e3
            assert rows_h == rows_d, (rows_h, rows_d)
            line += f", host parse path {out[f'q{i + 1}_host_ms']:.1f} ms (same rows)"
        print(line + f": {rows_d[:3]}{' ...' if len(rows_d) > 3 else ''}", flush=True)
    ctx.close()
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
