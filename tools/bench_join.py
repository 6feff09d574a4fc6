#!/usr/bin/env python3
"""Hash equi-join on the device: a fact batch of --rows rows (INT64 key, DOUBLE value, INT64 row id) probed against
dimension batches of several sizes (unique INT64 key = row index, DOUBLE value), both generated on the device with
qe_batch_generate.  The fact key is uniform in [0, 1.25 * build rows): about 80 % of the probe rows find their one match.
The output is (fact row id, fact value, dimension value).  Every call runs --warmup times unmeasured, then --reps times;
the best synchronised wall time around the ABI call is reported (the calls return after their own stream
synchronisation), next to the bytes each pass reads and writes by the model of DESIGN.md 3.8 and the time a plain read
stream of this run (qe_stream_read_bandwidth) would need for as many bytes.  --join-types lists the types every table is
probed with (INNER, LEFT, SEMI, ANTI, RIGHT, FULL; SEMI / ANTI without the dimension value).  --contention adds one table of
--contention build rows probed by a fact whose EVERY key is build row 0's: under RIGHT / FULL every probe row marks the same
build row.

    python tools/bench_join.py [--rows 100000000] [--build-rows 1000,1000000,16000000] [--join-types INNER] [--contention 0]
                               [--reps 5] [--warmup 1] [--json out.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from queryengine_amd import engine as E  # noqa: E402
from queryengine_amd import native as N  # noqa: E402


def spec(kind, col_id, modulus=0):
    s = N.GenSpec()
    s.kind, s.col_id, s.modulus = kind, col_id, modulus
    return s


def best_ms(ctx, call, reps, warmup, keep_last=False):
    times, last = [], None
    for i in range(warmup + reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        dt = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            times.append(dt)
        if keep_last and i == warmup + reps - 1:
            last = out
        else:
            out.free()
    return min(times), last


JOIN_TYPES = {"INNER": N.JOIN_INNER, "LEFT": N.JOIN_LEFT, "SEMI": N.JOIN_SEMI, "ANTI": N.JOIN_ANTI, "RIGHT": N.JOIN_RIGHT, "FULL": N.JOIN_FULL}


def dir_bits(m):
    b = 4
    while b < 26 and (1 << b) < m:
        b += 1
    return b


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--build-rows", default="1000,1000000,16000000")
    ap.add_argument("--join-types", default="INNER", help="comma-separated: " + ", ".join(JOIN_TYPES))
    ap.add_argument("--contention", type=int, default=0, help="build rows of one more table whose row 0 every probe row matches (0: none)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.rows
    ctx = E.Context(device=0)
    gbps = ctx.stream_read_bandwidth(1 << 30, 5)
    names = [t.strip().upper() for t in a.join_types.split(",")]
    out = {"probe_rows": n, "reps": a.reps, "warmup": a.warmup, "stream_read_gbps": gbps, "cases": []}
    print(f"hash equi-join on one device: {n} probe rows (INT64 key, DOUBLE value, INT64 row id) against unique INT64 build keys; "
          f"{', '.join(names)}, output = (probe row id, probe value, build value); best of {a.reps}, {a.warmup} warm-up run(s) excluded; "
          f"synchronised wall time around the call")
    print(f"qe_stream_read_bandwidth of this run: {gbps:.0f} GB/s")
    print(f"{'build rows':>11} {'type':>5} {'build ms':>9} {'probe ms':>9} {'output rows':>12} {'tail rows':>9} {'longest run':>11} | modelled MB read+written: "
          f"{'build':>8} {'pass 1':>8} {'pass 2':>8} {'gathers':>8} | {'probe MB':>9} {'as a stream, ms':>15} {'probe / stream':>14}")
    tables = [(int(v), False) for v in a.build_rows.split(",")] + ([(a.contention, True)] if a.contention > 0 else [])
    for nb, contended in tables:
        dim = E.DeviceBatch.generate(ctx, [spec(N.GEN_I64_ROWID, 0), spec(N.GEN_F64_UNIT, 1)], nb, seed=7)
        fact = E.DeviceBatch.generate(ctx, [spec(N.GEN_I64_MOD, 0, 1 if contended else nb + nb // 4), spec(N.GEN_F64_UNIT, 1), spec(N.GEN_I64_ROWID, 2)], n, seed=11)
        build_ms, table = best_ms(ctx, lambda: ctx.join_build(dim, [0]), a.reps, a.warmup, keep_last=True)
        for name in names:
            jt = JOIN_TYPES[name]
            build_out = [] if name in ("SEMI", "ANTI") else [1]
            probe_ms, res = best_ms(ctx, lambda: table.probe(fact, [0], jt, [2, 1], build_out), a.reps, a.warmup, keep_last=True)
            st = ctx.last_join_stats()
            rows_out = res.count
            tail = ctx.last_outer_stats()[2] if name in ("RIGHT", "FULL") else 0
            # the model of DESIGN.md 3.8 (bytes read + written)
            passes = (dir_bits(nb) + 3) // 4
            b_build = nb * (8 + 8 + 4 + 8) + passes * nb * (12 + 12 + 12) + ((1 << dir_bits(nb)) + 1) * 4 + nb * (4 + 4) + nb * (4 + 8 + 8)
            b_pass1 = n * 8 + n * 8 + n * 8 * (nb / (1 << dir_bits(nb))) + n * (4 + 4)     # key, two directory entries, the run's images, count + first
            b_pass2 = n * (4 + 4) + rows_out * (4 + 4 + 4)                                  # count + first, the build row of the match, the pair
            b_gather = rows_out * 3 * (4 + 8 + 8)                                           # per column: row id, value read, value written
            b_probe = b_pass1 + b_pass2 + b_gather
            stream_ms = b_probe / (gbps * 1e9) * 1e3
            out["cases"].append({"build_rows": nb, "join_type": name, "every_probe_row_on_build_row_0": contended, "tail_rows": tail,
                                 "build_ms": build_ms, "probe_ms": probe_ms, "output_rows": rows_out, "stats": st,
                                 "model_bytes": {"build": b_build, "pass1": b_pass1, "pass2": b_pass2, "gathers": b_gather},
                                 "probe_bytes_as_stream_ms": stream_ms})
            print(f"{nb:>11} {name:>5} {build_ms:>9.3f} {probe_ms:>9.3f} {rows_out:>12} {tail:>9} {st[3]:>11} | {'':>25} "
                  f"{b_build / 1e6:>8.1f} {b_pass1 / 1e6:>8.1f} {b_pass2 / 1e6:>8.1f} {b_gather / 1e6:>8.1f} | {b_probe / 1e6:>9.1f} {stream_ms:>15.3f} "
                  f"{probe_ms / stream_ms:>13.1f}x" + ("   <- every probe row matches build row 0" if contended else ""))
            res.free()
        table.free(); fact.free(); dim.free()
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
