#!/usr/bin/env python3
"""Range join of two results on the device (qe_result_range_join).  Both sides are generated on the device with
qe_batch_generate; the bounds of the left rows are made by a projection through qe_filter_project, as a caller would make them.
Every timing is synchronised wall time around the ABI call (the calls return after their own stream synchronisation); the
alternatives of a comparison alternate in one process, --warmup unmeasured rounds, then --reps measured ones, and every
measured round is listed below the tables.

1. The operator's own cost.  N rows a side, one INT32 by column of 1000 values, a DOUBLE `on` of uniform random times; every
   left row asks for [t, t + w] with w sized for about 1 and about 16 matches; INNER and LEFT; output = the INT64 row ids of
   both sides.  The yardstick is what the library already had: two qe_result_order_by_keys calls over 2 N rows of the same
   key types -- the two sorts the call runs on its own scratch copies of the keys.  The difference is the concatenations, the
   bitmaps, the ordinals, the scan, the expansion and the output gather.
2. The heavy hitter.  Equality written as a range (lo == hi, no by column) against qe_join_build + qe_join_probe on the same
   inputs: an INT64 key that holds one value on a quarter of the right rows and on 64 left rows, the other rows uniform; and
   the same sizes with every key uniform.  The two outputs are compared byte for byte before anything is timed.
3. Same output, different shape.  2^20 left rows against 2^24 right rows with the distinct values 0 .. 2^24 - 1, no by column,
   2^24 output rows: once every left row takes 16 of them, once one left row takes them all and the others ask for nothing.

--join-types lists the forms of parts 1 and 2 (INNER, LEFT, RIGHT, FULL); under RIGHT / FULL part 2 also compares the tails of
the two joins byte for byte.

    python tools/bench_range_join.py [--rows 1048576,4194304,16777216] [--join-types INNER,LEFT] [--reps 5] [--warmup 1]
                                     [--out profiles/range_join_summary.txt]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from queryengine_amd import ColumnExpression, DataType, Function, FunctionExpression, NumericLiteralExpression  # noqa: E402
from queryengine_amd import engine as E  # noqa: E402
from queryengine_amd import native as N  # noqa: E402

I32, I64, F64 = DataType.INT32, DataType.INT64, DataType.DOUBLE
INNER, LEFT = N.JOIN_INNER, N.JOIN_LEFT
JOIN_TYPES = {"INNER": INNER, "LEFT": LEFT, "RIGHT": N.JOIN_RIGHT, "FULL": N.JOIN_FULL}


def forms(a):
    return [(JOIN_TYPES[t.strip().upper()], t.strip().upper()) for t in a.join_types.split(",")]


def spec(kind, col_id, modulus=0, offset=0):
    s = N.GenSpec()
    s.kind, s.col_id, s.modulus, s.offset = kind, col_id, modulus, offset
    return s


def col(i, t):
    return ColumnExpression(f"c{i}", i, t)


def fn(f, a, b):
    return FunctionExpression(f, [a, b if not isinstance(b, float) else NumericLiteralExpression(b)], F64)


def generated(ctx, specs, nrows, seed, exprs):
    """A result of `exprs` over a generated batch."""
    batch = E.DeviceBatch.generate(ctx, specs, nrows, row_begin=0, seed=seed)
    res = E.filter_project(ctx, batch, None, [ctx.compile(e) for e in exprs])
    batch.free()
    return res


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    outs = call()
    dt = (time.perf_counter() - t0) * 1e3
    outs = outs if isinstance(outs, (list, tuple)) else [outs]
    count = outs[-1].count
    for o in outs:
        o.free()
    return dt, count


def rounds(ctx, calls, reps, warmup):
    """{name: [ms of every measured round]}, the calls alternating: who goes first changes every round."""
    ms = {name: [] for name, _ in calls}
    rows = {}
    for i in range(warmup + reps):
        for name, call in (calls if i % 2 == 0 else calls[::-1]):
            dt, rows[name] = timed(ctx, call)
            if i >= warmup:
                ms[name].append(dt)
    return ms, rows


def spread(v):
    return f"{min(v):.3f} .. {max(v):.3f}"


def column_bytes(result):
    return [(c.data.tobytes(), None if c.valid is None else c.valid.tobytes()) for c in result.to_columns()]


def own_cost(ctx, a, lines, runs):
    lines += ["1. the operator's own cost: N rows a side, INT32 by column of 1000 values, DOUBLE on, [t, t + w]; best of the rounds, ms",
              f"{'rows a side':>11} {'matches':>7} {'form':>5} {'range':>9} {'2 sorts':>9} {'range - 2 sorts':>15} {'rows out':>11} {'Mrows out / s':>13} {'longest':>7}"]
    for n in [int(v) for v in a.rows.split(",")]:
        keys_only = generated(ctx, [spec(N.GEN_I32_MOD, 0, 1000), spec(N.GEN_F64_UNIT, 7)], 2 * n, 29, [col(0, I32), col(1, F64)])
        right = generated(ctx, [spec(N.GEN_I32_MOD, 0, 1000), spec(N.GEN_F64_UNIT, 7), spec(N.GEN_I64_ROWID, 8)], n, 23, [col(0, I32), col(1, F64), col(2, I64)])
        for matches in (1, 16):
            w = matches * 1000.0 / n
            left = generated(ctx, [spec(N.GEN_I32_MOD, 0, 1000), spec(N.GEN_F64_UNIT, 7), spec(N.GEN_I64_ROWID, 8)], n, 17,
                             [col(0, I32), col(1, F64), fn(Function.ADD, col(1, F64), w), col(2, I64)])
            for join_type, form in forms(a):
                calls = [("range", lambda: ctx.range_join(left, right, [0], [0], 1, 2, 1, False, False, join_type, [3], [2])),
                         ("sorts", lambda: [ctx.order_by_keys(keys_only, [(0, False), (1, False)]) for _ in range(2)])]
                ms, rows = rounds(ctx, calls, a.reps, a.warmup)
                ctx.range_join(left, right, [0], [0], 1, 2, 1, False, False, join_type, [3], [2]).free()
                stats = ctx.last_range_stats()
                r, s = min(ms["range"]), min(ms["sorts"])
                lines.append(f"{n:>11} {matches:>7} {form:>5} {r:>9.3f} {s:>9.3f} {r - s:>15.3f} {rows['range']:>11} {rows['range'] / r / 1e3:>13.1f} {stats['longest']:>7}")
                runs.append(f"1. {n} rows, {matches} matches, {form}: range {' '.join(f'{v:.3f}' for v in ms['range'])} | 2 sorts {' '.join(f'{v:.3f}' for v in ms['sorts'])}")
            left.free()
        right.free()
        keys_only.free()
        ctx.trim()


def heavy_hitter(ctx, a, lines, runs):
    n, keys = 1 << 20, 1 << 20
    lines += ["", f"2. equality as a range against the hash join: {n} rows a side, INT64 key, output = the INT64 row ids of both sides; best of the rounds, ms",
              f"{'keys':>30} {'form':>5} {'range':>9} {'build + probe':>13} {'range / hash':>12} {'rows out':>11} {'longest':>8}"]

    def side(heavy_rows, seed):
        exprs = [col(0, I64), col(1, I64)]
        if heavy_rows == 0:
            return generated(ctx, [spec(N.GEN_I64_MOD, 0, keys, 1), spec(N.GEN_I64_ROWID, 8)], n, seed, exprs)
        parts = [generated(ctx, [spec(N.GEN_I64_MOD, 0, 1), spec(N.GEN_I64_ROWID, 8)], heavy_rows, seed, exprs),       # key 0
                 generated(ctx, [spec(N.GEN_I64_MOD, 0, keys, 1), spec(N.GEN_I64_ROWID, 8)], n - heavy_rows, seed + 1, exprs)]
        whole = ctx.concat(parts)
        for p in parts:
            p.free()
        return whole

    for name, lheavy, rheavy in (("one key on 1/4 of the right rows", 64, n // 4), ("uniform", 0, 0)):
        left, right = side(lheavy, 17), side(rheavy, 23)
        for join_type, form in forms(a):
            def hashed():
                table = ctx.join_build(right, [0])
                try:
                    return table.probe(left, [0], join_type, [1], [1])
                finally:
                    table.free()

            def ranged():
                return ctx.range_join(left, right, [], [], 0, 0, 0, False, False, join_type, [1], [1])
            h, r = hashed(), ranged()
            same = column_bytes(h) == column_bytes(r)
            h.free()
            r.free()
            longest = ctx.last_range_stats()["longest"]
            if not same:
                raise SystemExit(f"the range join and the hash join differ: {name} {form}")
            ms, rows = rounds(ctx, [("range", ranged), ("hash", hashed)], a.reps, a.warmup)
            r, h = min(ms["range"]), min(ms["hash"])
            lines.append(f"{name:>30} {form:>5} {r:>9.3f} {h:>13.3f} {r / h:>12.2f} {rows['range']:>11} {longest:>8}")
            runs.append(f"2. {name}, {form} (equal bytes): range {' '.join(f'{v:.3f}' for v in ms['range'])} | build + probe {' '.join(f'{v:.3f}' for v in ms['hash'])}")
        left.free()
        right.free()
        ctx.trim()


def same_output(ctx, a, lines, runs):
    nl, nr, per = 1 << 20, 1 << 24, 16.0
    lines += ["", f"3. same output, different shape: {nl} left rows, {nr} right rows of distinct DOUBLE values, no by column, INNER, {nr} output rows; ms",
              f"{'shape':>34} {'best':>9} {'rounds':>21} {'rows out':>11} {'longest':>9}"]
    rowid = col(0, I64)
    right = generated(ctx, [spec(N.GEN_I64_ROWID, 8)], nr, 23, [fn(Function.MUL, rowid, 1.0), rowid])
    lo = fn(Function.MUL, rowid, per)
    uniform = generated(ctx, [spec(N.GEN_I64_ROWID, 8)], nl, 17, [lo, fn(Function.ADD, lo, per - 1.0), rowid])
    # The rows that ask for nothing hold the reversed interval [1, 0], not negative bounds: the image of a negative double has
    # all its low bits set, which would make the sort run every radix pass where the other shape skips the constant low digits,
    # and the comparison would measure the sort, not the expansion.
    zero = fn(Function.MUL, rowid, 0.0)
    parts = [generated(ctx, [spec(N.GEN_I64_ROWID, 8)], 1, 17, [zero, fn(Function.ADD, zero, float(nr - 1)), rowid]),          # [0, nr - 1]
             generated(ctx, [spec(N.GEN_I64_ROWID, 8)], nl - 1, 18, [fn(Function.ADD, zero, 1.0), zero, rowid])]               # [1, 0]
    skewed = ctx.concat(parts)
    for p in parts:
        p.free()
    calls = [(name, lambda left=left: ctx.range_join(left, right, [], [], 0, 1, 0, False, False, INNER, [2], [1]))
             for name, left in (("16 matches on every left row", uniform), ("all matches on one left row", skewed))]
    ms, rows = rounds(ctx, calls, a.reps, a.warmup)
    for name, call in calls:
        call().free()
        lines.append(f"{name:>34} {min(ms[name]):>9.3f} {spread(ms[name]):>21} {rows[name]:>11} {ctx.last_range_stats()['longest']:>9}")
        runs.append(f"3. {name}: {' '.join(f'{v:.3f}' for v in ms[name])}")
    for r in (uniform, skewed, right):
        r.free()
    ctx.trim()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="1048576,4194304,16777216", help="rows per side of part 1, one run of every case each")
    ap.add_argument("--join-types", default="INNER,LEFT", help="forms of parts 1 and 2, comma-separated: " + ", ".join(JOIN_TYPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args()
    ctx = E.Context(device=0)
    lines = [f"range join of two results on one device: {a.reps} measured rounds after {a.warmup} warm-up round(s), the alternatives of a comparison "
             "alternating in one process; synchronised wall time around the ABI call(s)", ""]
    runs = ["every measured round (ms):"]
    for part, run in (("1", own_cost), ("2", heavy_hitter), ("3", same_output)):
        if part in a.parts.split(","):
            run(ctx, a, lines, runs)
    ctx.close()
    text = "\n".join(lines + [""] + runs)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
