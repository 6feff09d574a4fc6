"""CSV parsed on the device (qe_csv_parse_device / qe_csv_parse_file_device) against the host path (qe_csv_parse +
qe_csv_pin): the same batch -- bit-equal doubles, equal codes and dictionaries, equal value and validity bits, equal
nullability -- or the same error."""
import ctypes as C
import math
import random

import numpy as np
import pytest

from queryengine_amd import DataType, Field, Schema
from queryengine_amd.csv_table import CsvColumnarTable, DeviceCsvTable, read_csv_device, read_csv_native

pytestmark = pytest.mark.gpu

S, D, B = DataType.STRING, DataType.DOUBLE, DataType.BOOLEAN

# the fixtures of tests/test_csv_table.py (copied)
CSV = '''id,country,price,paid,note
1,DE,100.5,true,"hello, world"

2,"AT",  2.5e1 ,TRUE,"say ""hi"""
3,,NaN,false,
4,CH,0x1p3,yes
5,DE,-Infinity,,x
6,DE,7d,False,y,extra
'''
MORE = ("id,country,price,paid,note\r\n"
        '7,"multi\nline",1e-3,true,"a,b"\r\n'
        "\r\n"
        '8,Zürich \U0001F600,+.5,tRuE,""\r'
        "9,,Infinity,,last")
SCHEMA = Schema([Field("id", S), Field("country", S), Field("price", D), Field("paid", B), Field("note", S)])


def stats(ctx):
    from queryengine_amd import native as N
    s = N.CsvDeviceStats()
    N.check(ctx.handle, ctx._lib.qe_csv_device_last_stats(ctx.handle, C.byref(s)))
    return s


def host_batch(ctx, src, schema, proj):
    """(batch, dictionaries) of qe_csv_parse + qe_csv_pin, or the exception"""
    try:
        t = read_csv_native(ctx, src, schema, proj)
    except Exception as e:   # noqa: BLE001 -- compared with the device path's
        return e
    return t.native.pin(), [c.dictionary for c in t.columns]


def check_parity(ctx, src, schema, proj=None, fallback=0):
    want = host_batch(ctx, src, schema, proj)
    if isinstance(want, Exception):
        with pytest.raises(type(want)) as got:
            read_csv_device(ctx, src, schema, proj)
        assert str(got.value) == str(want)
        assert stats(ctx).host_fallback == 1
        return None
    hb, hdicts = want
    dev = read_csv_device(ctx, src, schema, proj)
    db = dev.batch
    st = stats(ctx)
    assert st.host_fallback == fallback, (st.host_fallback, fallback)
    assert db.nrows == hb.nrows == st.nrows and db.ncols == hb.ncols
    n = hb.nrows
    for j in range(hb.ncols):
        assert db.column_type(j) == hb.column_type(j)
        assert ctx._lib.qe_batch_column_nullable(db.handle, j) == ctx._lib.qe_batch_column_nullable(hb.handle, j), j
        assert dev.dictionaries[j] == hdicts[j], j
        if n == 0:
            continue
        t = hb.column_type(j)
        nw = (n + 63) // 64
        outs = []
        for b in (db, hb):
            data = np.zeros(nw if t == B else n, dtype=np.uint64 if t in (B, D) else np.int32)
            valid = np.zeros(nw, dtype=np.uint64)
            from queryengine_amd import native as N
            N.check(ctx.handle, ctx._lib.qe_batch_column_to_host(ctx.handle, b.handle, j, 0, n, data.ctypes.data, valid.ctypes.data))
            outs.append((data, valid))
        assert np.array_equal(outs[0][1], outs[1][1]), f"validity of column {j}"
        bad = np.nonzero(outs[0][0] != outs[1][0])[0]
        assert bad.size == 0, f"column {j}: first difference at {bad[:5]}: {outs[0][0][bad[:5]]} != {outs[1][0][bad[:5]]}"
    hb.free()
    db.free()
    return st


def test_fixtures(gpu_ctx, tmp_path):
    for k, text in enumerate((CSV, MORE)):
        p = tmp_path / f"t{k}.csv"
        p.write_bytes(text.encode("utf-8"))
        for proj in (None, ["price", "id"], ["note", "paid", "country"], ["paid", "paid"], []):
            for src in (text.encode("utf-8"), str(p)):
                check_parity(gpu_ctx, src, SCHEMA, proj)
    dup = b"x,y,x\n1,2,3\n4,5,\n"
    check_parity(gpu_ctx, dup, Schema([Field("x", D), Field("y", D)]))
    ok = b"price\n 0x1.8p1 \n7D\n-NaN\n1e400\n-0\n123456789012345678901234567\n"
    st = check_parity(gpu_ctx, ok, Schema([Field("price", D)]))
    assert st.host_patched_fields == 2          # the hexadecimal literal and the 27-digit one
    for text in (b"", b"\n\n", b"a,b\n", b"a,b", b"a,b\r\n\r\n", b"\r\na,b\n1,2", b"a,b\n,\n", b"a,b\n1,", b"a\n\"\"\n"):
        check_parity(gpu_ctx, text, Schema([Field("a", S), Field("b", D)]), ["a"])
        check_parity(gpu_ctx, text, Schema([Field("a", S)]), [])


def test_fallback_inputs(gpu_ctx):
    sch = Schema([Field("a", S), Field("b", D)])
    cases = [b'a,b\nab"c,1\n',              # a quote inside an unquoted field: text for the host
             b'a,b\n"ab"x,1\n',             # a character after a closing quote: the host's error
             b'a,b\n"ab,1\n',               # unterminated quote
             b'a,b\nx,1.5.5\n',             # NumberFormatException
             b'a,b\nx,"1""5"\n',
             b'c,d\n1,2\n',                 # a projected name missing from the header
             b'',                           # no header at all
             "\ufeffa,b\n1,2\n".encode("utf-8")]   # a byte order mark stays part of the first name
    for text in cases:
        check_parity(gpu_ctx, text, sch, fallback=1)
    check_parity(gpu_ctx, b'a,b\nab"c,1\n', sch, ["b"], fallback=1)


def rand_field(rng, kind):
    r = rng.random()
    if r < 0.08:
        return ""
    if kind == "s":
        pool = ["DE", "AT", "CH", "Zürich \U0001F600", "a,b", "multi\nline", "cr\rlf\r\n", 'say "hi"', "x" * rng.randint(1, 40),
                "", " ", "été", str(rng.randint(0, 50))]
        s = rng.choice(pool)
    elif kind == "d":
        forms = [f"{rng.uniform(-1e3, 1e3):.2f}", repr(rng.uniform(-1e300, 1e300)), repr(rng.random() * 1e-310), "NaN", "-NaN",
                 "Infinity", "-Infinity", f" {rng.randint(0, 99)} ", f"{rng.randint(0, 9)}d", f"{rng.randint(0, 9)}.5F", ".5", "5.",
                 "-0", "1e400", "0x1.8p1", f"{rng.random():.24f}", f"{rng.randint(0, 10**6)}e-{rng.randint(0, 30)}"]
        s = rng.choice(forms)
    else:
        s = rng.choice(["true", "TRUE", "tRuE", "false", "yes", "1", "true ", "truee"])
    if any(c in s for c in ',\n\r"') or rng.random() < 0.2:
        return '"' + s.replace('"', '""') + '"'
    return s


def rand_text(rng, nrows, kinds, header):
    eols = ["\n", "\r\n", "\r"]
    out = [",".join(header) + rng.choice(eols)]
    for _ in range(nrows):
        if rng.random() < 0.03:
            out.append(rng.choice(eols))                       # an empty line
        k = len(kinds)
        r = rng.random()
        if r < 0.05:
            k = rng.randint(1, len(kinds))                     # a short record
        fields = [rand_field(rng, kinds[i]) for i in range(k)]
        if r > 0.95:
            fields += [rand_field(rng, "s") for _ in range(rng.randint(1, 3))]   # a long one
        out.append(",".join(fields) + rng.choice(eols))
    if rng.random() < 0.5:
        out[-1] = out[-1].rstrip("\r\n")
    return "".join(out)


KINDS = ["s", "d", "b", "d", "s", "b", "d"]
HEADER = ["s0", "d0", "b0", "d1", "s1", "b1", "d2"]
RSCHEMA = Schema([Field(h, {"s": S, "d": D, "b": B}[k]) for h, k in zip(HEADER, KINDS)])


def test_random_inputs(gpu_ctx, tmp_path):
    rng = random.Random(7)
    for it in range(40):
        text = rand_text(rng, rng.choice([1, 5, 63, 64, 65, 300, 2000]), KINDS, HEADER)
        proj = rng.sample(HEADER, rng.randint(1, len(HEADER)))
        st = check_parity(gpu_ctx, text.encode("utf-8"), RSCHEMA, proj)
        assert st is not None and st.host_fallback == 0


def test_boundaries_and_sizes(gpu_ctx, tmp_path):
    sch = Schema([Field("a", S), Field("b", D)])
    # a record, a quoted newline and a \r\n pair across the 4 KiB tiles of the structure passes
    for off in (4093, 4094, 4095, 4096, 4097, 8191, 8192, 3 * 4096 - 1):
        for tail in ('"x\ny",1.5\r\n', 'q,2\r\nr,3\r\n', '"a""b",4\n\n', '"\r\n",5\r'):
            pad = "p," + "7" * max(1, off - 6) + "\n"
            check_parity(gpu_ctx, ("a,b\n" + pad + tail + "z,9\n").encode(), sch)
    # large texts: a random block repeated (block length not a multiple of a tile), up to a few hundred MB, from bytes and
    # from a file (the file is read in 64 MiB chunks)
    rng = random.Random(11)
    block = rand_text(rng, 20000, KINDS, HEADER).split("\n", 1)[1]
    block = block.rstrip("\r\n") + "\n"
    for reps, via_file in ((3, False), (40, True), (150, False)):
        text = (",".join(HEADER) + "\n" + block * reps).encode("utf-8")
        src = text
        if via_file:
            p = tmp_path / "big.csv"
            p.write_bytes(text)
            src = str(p)
        st = check_parity(gpu_ctx, src, RSCHEMA, ["s0", "d1", "b1", "s1"])
        assert st.host_fallback == 0 and st.text_bytes == len(text)


def tripdata_text(nrows, seed):
    """tripdata-shaped records (the 2019-01 header, 18 fields, the number forms of the real file)"""
    rng = random.Random(seed)
    out = ["VendorID,tpep_pickup_datetime,tpep_dropoff_datetime,passenger_count,trip_distance,RatecodeID,store_and_fwd_flag,"
           "PULocationID,DOLocationID,payment_type,fare_amount,extra,mta_tax,tip_amount,tolls_amount,improvement_surcharge,"
           "total_amount,congestion_surcharge\n"]
    for _ in range(nrows):
        fare = rng.randrange(0, 30000) / 100 * rng.choice([1, 1, 1, -1])
        tip = round(abs(fare) * rng.choice([0, 0.1, 0.15, 0.2]), 2)
        f = lambda v: f"{v:g}" if rng.random() < 0.5 else f"{v}"
        out.append(f"{rng.choice([1, 2])},2019-01-{rng.randint(1, 31):02d} 00:46:40,2019-01-01 00:53:20,{rng.randint(0, 9)},"
                   f"{rng.randrange(0, 5000) / 100:.2f},{rng.choice([1, 2, 5, 99])},{rng.choice('NY')},{rng.randint(1, 265)},"
                   f"{rng.randint(1, 265)},{rng.randint(1, 4)},{f(fare)},0.5,0.5,{f(tip)},{rng.choice(['0', '5.76'])},0.3,"
                   f"{f(round(fare + tip + 1.3, 2))},{rng.choice(['', '', '2.5'])}\n")
    return "".join(out).encode()


def test_tripdata_shape_needs_no_patches(gpu_ctx):
    text = tripdata_text(20_000, seed=3)
    names = text.split(b"\n", 1)[0].decode().split(",")
    sch = Schema([Field(n, S if n in ("tpep_pickup_datetime", "tpep_dropoff_datetime", "store_and_fwd_flag") else D) for n in names])
    for proj in (["tip_amount", "fare_amount", "passenger_count"], None):
        st = check_parity(gpu_ctx, text, sch, proj)
        assert st.host_fallback == 0 and st.host_patched_fields == 0


def test_queries_over_device_csv_table(gpu_ctx, tmp_path):
    from queryengine_amd.planner import Mode, query
    rng = random.Random(5)
    text = rand_text(rng, 3000, ["s", "d", "b", "d"], ["k", "x", "f", "y"])
    p = tmp_path / "q.csv"
    p.write_bytes(text.encode("utf-8"))
    sch = Schema([Field("k", S), Field("x", D), Field("f", B), Field("y", D)])
    host, dev = CsvColumnarTable(str(p), sch), DeviceCsvTable(str(p), sch)
    dev_bytes = DeviceCsvTable(text.encode("utf-8"), sch)
    sqls = ["SELECT k, x * 2 FROM t WHERE f AND x < 500",
            "SELECT MIN(x), MAX(x), COUNT(y) FROM t",
            "SELECT k, COUNT(x), MIN(y) FROM t",
            "SELECT y, COUNT(k) FROM t WHERE y > -1000 AND y < 1000",
            "SELECT k, y FROM t WHERE y >= 0 ORDER BY 2"]

    def same(a, b):
        if isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b):
            return True
        return a == b
    for sql in sqls:
        want = query("t", sql, Mode.GPU_FUSED, table=host, ctx=gpu_ctx)
        for t in (dev, dev_bytes):
            got = query("t", sql, Mode.GPU_FUSED, table=t, ctx=gpu_ctx)
            assert len(got) == len(want) and all(len(g) == len(w) and all(same(x, y) for x, y in zip(g, w))
                                                 for g, w in zip(got, want)), sql
    # the row source of the scan leaf
    op = dev.getScanOperator(["k", "x"])
    op.device_batch(gpu_ctx)
    op.open()
    ref = host.getScanOperator(["k", "x"])
    ref.open()
    for _ in range(50):
        a, b = op.next(), ref.next()
        assert a is not None and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
