#!/usr/bin/env python3
"""Set operations over two results on the device: two results of --rows rows each (INT64 row id, DOUBLE of 1000 distinct
values, dictionary STRING of 16 entries), generated on the device with qe_batch_generate and an identity projection, go through
qe_result_set_op in all six forms.  The right side is the generator's rows [(1 - overlap) * rows, (2 - overlap) * rows), so
`overlap` of its tuples also stand on the left; both sides carry one dictionary object.

The yardstick for UNION is what the library could already do with the same rows: qe_result_concat followed by
qe_result_group_ordered over every column with no function (SELECT DISTINCT).  Both run the same sort and UNION does less
after it, so UNION is expected not to be slower than the composition by more than the spread (max - min) that the
composition's own repeated runs show in this call.  The two alternate in one process, after --warmup unmeasured rounds, for
--reps rounds; which of the two goes first changes every round, and every single time is printed.  Every other form runs
--warmup times unmeasured, then --reps times; times are synchronised wall time around the ABI call (the calls return after
their own stream synchronisation).  One more line times UNION with a right side whose dictionary holds the same entries in
another order, which adds the translation of the right side's codes.

    python tools/bench_setop.py [--rows 67108864] [--overlap 0,0.5,1] [--reps 8] [--warmup 1] [--out profiles/setop_summary.txt]"""
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
FORMS = [(N.SET_UNION, False, "UNION"), (N.SET_UNION, True, "UNION ALL"), (N.SET_INTERSECT, False, "INTERSECT"),
         (N.SET_INTERSECT, True, "INTERSECT ALL"), (N.SET_EXCEPT, False, "EXCEPT"), (N.SET_EXCEPT, True, "EXCEPT ALL")]


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
    ap.add_argument("--rows", type=int, default=1 << 26, help="rows per side")
    ap.add_argument("--overlap", default="0,0.5,1")
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    n = a.rows
    ctx = E.Context(device=0)
    words, reordered = ctx.dictionary(WORDS), ctx.dictionary(WORDS[::-1])
    types = [DataType.INT64, DataType.DOUBLE, DataType.STRING]
    projs = [ctx.compile(ColumnExpression(f"c{i}", i, t)) for i, t in enumerate(types)]

    def side(row_begin, dictionary):
        batch = E.DeviceBatch.generate(ctx, [spec(N.GEN_I64_ROWID, 0), spec(N.GEN_F64_MOD, 1, 1000), spec(N.GEN_DICT_MOD, 2, len(WORDS), dictionary)],
                                       n, row_begin=row_begin, seed=17)
        res = E.filter_project(ctx, batch, None, projs)
        return batch, res

    def composition(left, right):
        cat = ctx.concat([left, right])
        try:
            return ctx.group_ordered(cat, [0, 1, 2], [])
        finally:
            cat.free()

    lines = [f"set operations of two results on one device: {n} rows a side (INT64 row id, DOUBLE of 1000 values, STRING of {len(WORDS)} entries, one "
             f"dictionary object); {a.reps} measured runs after {a.warmup} warm-up run(s); synchronised wall time around the call, ms",
             f"{'overlap':>7} {'form':>14} {'best':>9} {'median':>9} {'rows out':>11} {'tuples':>11}"]
    union_lines = ["UNION against qe_result_concat + qe_result_group_ordered (no function), alternating in one process:",
                   f"{'overlap':>7} {'UNION best':>11} {'comp best':>10} {'comp worst':>10} {'comp spread':>11} {'UNION - comp':>12} {'within spread':>13}"]
    runs = ["every measured round (ms):"]
    lbatch, left = side(0, words)
    for overlap in [float(v) for v in a.overlap.split(",")]:
        begin = int(round((1.0 - overlap) * n))
        rbatch, right = side(begin, words)
        # UNION and its yardstick, alternating
        u_ms, c_ms = [], []
        for i in range(a.warmup + a.reps):
            if i % 2 == 0:      # who goes first changes every round: neither always inherits the other's pool and clocks
                dc, comp_rows = timed(ctx, lambda: composition(left, right))
                du, union_rows = timed(ctx, lambda: ctx.set_op(left, right, N.SET_UNION, False))
            else:
                du, union_rows = timed(ctx, lambda: ctx.set_op(left, right, N.SET_UNION, False))
                dc, comp_rows = timed(ctx, lambda: composition(left, right))
            assert comp_rows == union_rows, (comp_rows, union_rows)
            if i >= a.warmup:
                c_ms.append(dc)
                u_ms.append(du)
        spread = max(c_ms) - min(c_ms)
        diff = min(u_ms) - min(c_ms)
        union_lines.append(f"{overlap:>7.2f} {min(u_ms):>11.3f} {min(c_ms):>10.3f} {max(c_ms):>10.3f} {spread:>11.3f} {diff:>12.3f} "
                           f"{'yes' if diff <= spread else 'NO':>13}")
        runs.append(f"{overlap:>7.2f} UNION {' '.join(f'{v:.3f}' for v in u_ms)} | composition {' '.join(f'{v:.3f}' for v in c_ms)}")
        for op, all_, name in FORMS:
            ms = []
            for i in range(a.warmup + a.reps):
                dt, rows = timed(ctx, lambda: ctx.set_op(left, right, op, all_))
                if i >= a.warmup:
                    ms.append(dt)
            st = ctx.last_set_stats()
            lines.append(f"{overlap:>7.2f} {name:>14} {min(ms):>9.3f} {sorted(ms)[len(ms) // 2]:>9.3f} {rows:>11} {st['tuples']:>11}")
        right.free(); rbatch.free()
    # the translation of the right side's codes: the same entries in another order
    rbatch, right = side(n // 2, reordered)
    ms = []
    for i in range(a.warmup + a.reps):
        dt, rows = timed(ctx, lambda: ctx.set_op(left, right, N.SET_UNION, False))
        if i >= a.warmup:
            ms.append(dt)
    assert ctx.last_set_stats()["translated_columns"] == 1
    tail = f"UNION with the right dictionary reordered (codes translated on the device), generator rows from {n // 2}: best {min(ms):.3f} ms, {rows} rows out"
    right.free(); rbatch.free(); left.free(); lbatch.free()
    ctx.close()
    text = "\n".join(lines + [""] + union_lines + runs + ["", tail])
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
