#!/usr/bin/env python3
"""ASOF join of two results on the device: two results of --rows rows each, generated on the device with qe_batch_generate and
an identity projection, go through qe_result_asof_join (by columns, a DOUBLE `on` of uniform random times, an INT64 row id as
the one output column of either side).  The two sides draw from different random streams, so their times interleave.

Cases: 1 by column (INT32 of 1000 values), 3 by columns (INT32 of 10, INT64 of 10, dictionary STRING of 16 entries on one
dictionary object: 1600 partitions), and 1 STRING by column whose right side carries the same entries in another order (a
merged dictionary, the right codes translated on the device).  Forms: BACKWARD not strict as LEFT and as INNER, FORWARD strict
as LEFT.

The yardstick is what the library already had for the same number of rows and the same key types: qe_result_order_by_keys
over a result of 2 * rows rows that holds the key columns only, by all of them.  The ASOF call runs that sort on its own
scratch copy of the keys and adds the concatenation, the boundary flags, its bitmaps, the pick and the output gather; the
difference of the two times is the operator's own cost.  The two alternate in one process, after --warmup unmeasured rounds,
for --reps rounds; times are synchronised wall time around the ABI call (the calls return after their own stream
synchronisation).

    python tools/bench_asof.py [--rows 4194304,33554432,134217728] [--reps 5] [--warmup 1] [--out profiles/asof_summary.txt]"""
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

WORDS = [f"w{i:02d}" for i in range(16)]
I32, I64, F64, STR = DataType.INT32, DataType.INT64, DataType.DOUBLE, DataType.STRING
FORMS = [(N.ASOF_BACKWARD, False, N.JOIN_LEFT, "BACKWARD LEFT"), (N.ASOF_BACKWARD, False, N.JOIN_INNER, "BACKWARD INNER"),
         (N.ASOF_FORWARD, True, N.JOIN_LEFT, "FORWARD strict LEFT")]


def spec(kind, col_id, modulus=0, dictionary=None):
    s = N.GenSpec()
    s.kind, s.col_id, s.modulus = kind, col_id, modulus
    if dictionary is not None:
        s.dict = dictionary.handle
    return s


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = call()
    dt = (time.perf_counter() - t0) * 1e3
    count = out.count
    out.free()
    return dt, count


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="4194304,33554432,134217728", help="rows per side, one run of every case each")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    ctx = E.Context(device=0)
    words, reordered = ctx.dictionary(WORDS), ctx.dictionary(WORDS[::-1])
    # (name, by column types, generator specs of the by columns given the STRING dictionary of the side, right dictionary)
    cases = [("1 by (INT32)", [I32], lambda d: [spec(N.GEN_I32_MOD, 0, 1000)], words),
             ("3 by (INT32, INT64, STRING)", [I32, I64, STR], lambda d: [spec(N.GEN_I32_MOD, 0, 10), spec(N.GEN_I64_MOD, 1, 10), spec(N.GEN_DICT_MOD, 2, len(WORDS), d)], words),
             ("1 by (STRING, dictionaries differ)", [STR], lambda d: [spec(N.GEN_DICT_MOD, 2, len(WORDS), d)], reordered)]
    lines = [f"ASOF join of two results on one device: DOUBLE `on` of uniform random times, INT64 row id out of either side; {a.reps} measured rounds "
             f"after {a.warmup} warm-up round(s), the ASOF call and qe_result_order_by_keys over the same number of rows and key types alternating; "
             "synchronised wall time around the call, best of the rounds, ms",
             f"{'rows a side':>11} {'case':>34} {'form':>19} {'asof':>9} {'sort':>9} {'asof - sort':>11} {'rows out':>11} {'partitions':>10}"]
    runs = ["every measured round (ms):"]
    for n in [int(v) for v in a.rows.split(",")]:
        for name, by_types, by_specs, right_dict in cases:
            nby = len(by_types)
            types = by_types + [F64, I64]
            projs = [ctx.compile(ColumnExpression(f"c{i}", i, t)) for i, t in enumerate(types)]

            def side(nrows, seed, dictionary, with_rowid=True):
                specs = by_specs(dictionary) + [spec(N.GEN_F64_UNIT, 7)] + ([spec(N.GEN_I64_ROWID, 8)] if with_rowid else [])
                batch = E.DeviceBatch.generate(ctx, specs, nrows, row_begin=0, seed=seed)
                res = E.filter_project(ctx, batch, None, projs[:len(specs)])
                batch.free()
                return res

            left, right = side(n, 17, words), side(n, 23, right_dict)
            keys_only = side(2 * n, 29, words, with_rowid=False)           # the yardstick's input: 2 n rows of the key columns
            sort_keys = [(c, False) for c in range(nby + 1)]
            by = list(range(nby))
            for direction, strict, join_type, form in FORMS:
                a_ms, s_ms = [], []
                for i in range(a.warmup + a.reps):
                    calls = [("a", lambda: ctx.asof_join(left, right, by, by, nby, nby, direction, strict, join_type, [nby + 1], [nby + 1])),
                             ("s", lambda: ctx.order_by_keys(keys_only, sort_keys))]
                    for which, call in (calls if i % 2 == 0 else calls[::-1]):     # who goes first changes every round
                        dt, rows = timed(ctx, call)
                        if which == "a":
                            rows_out, stats = rows, ctx.last_asof_stats()
                        if i >= a.warmup:
                            (a_ms if which == "a" else s_ms).append(dt)
                lines.append(f"{n:>11} {name:>34} {form:>19} {min(a_ms):>9.3f} {min(s_ms):>9.3f} {min(a_ms) - min(s_ms):>11.3f} {rows_out:>11} "
                             f"{stats['partitions']:>10}")
                runs.append(f"{n:>11} {name} {form}: asof {' '.join(f'{v:.3f}' for v in a_ms)} | sort {' '.join(f'{v:.3f}' for v in s_ms)}")
            for r in (left, right, keys_only):
                r.free()
            ctx.trim()
    ctx.close()
    text = "\n".join(lines + [""] + runs)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
