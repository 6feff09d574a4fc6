"""The device CSV parser without a device: its C ABI, and its decimal -> double converter (qe_csv_number.h) compiled for the
host and checked bit for bit against the host parser (java_parse_double = the Java grammar + strtod) on > 10^6 strings."""
import ctypes as C
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from csv_number_corpus import corpus, undecidable
from queryengine_amd import DataType, Field, Schema
from queryengine_amd import native as N
from queryengine_amd.csv_table import NumberFormatException, java_parse_double

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "queryengine_amd", "csrc")
NEW = ("qe_csv_parse_device", "qe_csv_parse_file_device", "qe_csv_device_last_stats", "qe_batch_column_nullable",
       "qe_batch_column_dict")
OK, REJECT, UNDECIDED = 0, 1, 2

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "qe_csv_number.h"
// stdin: records {u32 length, bytes}; stdout: records {u64 status, u64 bits}
int main() {
    unsigned len;
    std::vector<unsigned char> buf;
    while (std::fread(&len, 4, 1, stdin) == 1) {
        buf.resize(len + 1);
        if (len && std::fread(buf.data(), 1, len, stdin) != len) return 1;
        double v = 0.0;
        unsigned long long rec[2] = {(unsigned long long)qe_parse_double(buf.data(), len, v), 0};
        if (rec[0] == QE_NUM_OK) std::memcpy(&rec[1], &v, 8);
        std::fwrite(rec, 8, 2, stdout);
    }
    return 0;
}
"""


def test_new_symbols_are_declared_exported_and_bound(native_lib):
    header = open(os.path.join(ROOT, "include", "qe_hip.h")).read()
    bound = {n for n, _, _ in N.SYMBOLS}
    for name in NEW:
        assert f"{name}(" in header and hasattr(native_lib, name) and name in bound, name


def test_planning_only_context_has_no_cpu_path(native_lib, tmp_path):
    from queryengine_amd import engine as E
    ctx = E.Context(device=None, jit_cache_dir=str(tmp_path / "jit"))
    names = (C.c_char_p * 1)(b"a")
    types = (C.c_int32 * 1)(int(DataType.DOUBLE))
    h = C.c_void_p()
    st = native_lib.qe_csv_parse_device(ctx.handle, b"a\n1\n", 4, 1, names, types, C.byref(h))
    assert st == 3 and not h and b"planning-only" in native_lib.qe_last_error(ctx.handle)
    p = tmp_path / "a.csv"
    p.write_bytes(b"a\n1\n")
    st = native_lib.qe_csv_parse_file_device(ctx.handle, str(p).encode(), 1, names, types, C.byref(h))
    assert st == 3 and not h
    s = N.CsvDeviceStats()
    assert native_lib.qe_csv_device_last_stats(ctx.handle, C.byref(s)) == 0 and s.host_fallback == 0
    ctx.close()


def test_pow5_table_is_the_generators_output():
    assert subprocess.run(["python3", os.path.join(ROOT, "tools", "gen_pow5_table.py"), "--check"]).returncode == 0


@pytest.fixture(scope="module")
def converter(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("num")
    (d / "drv.cpp").write_text(DRIVER)
    exe = d / "drv"
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, str(d / "drv.cpp"), "-o", str(exe)], check=True)

    def run(strings):
        data = b"".join(struct.pack("<I", len(s)) + s for s in (x.encode("latin-1") for x in strings))
        out = subprocess.run([str(exe)], input=data, stdout=subprocess.PIPE, check=True).stdout
        rec = np.frombuffer(out, dtype=np.uint64).reshape(-1, 2)
        assert rec.shape[0] == len(strings)
        return rec[:, 0].astype(np.int64), rec[:, 1].copy()
    return run


def host_values(strings, tmp_path):
    """The host parser (qe_csv_parse, java_parse_double) on one DOUBLE column holding the strings."""
    from queryengine_amd import engine as E
    from queryengine_amd.csv_table import read_csv_native
    ctx = E.Context(device=None, jit_cache_dir=str(tmp_path / "jit"))
    text = ("x\n" + "\n".join(strings) + "\n").encode("latin-1")
    t = read_csv_native(ctx, text, Schema([Field("x", DataType.DOUBLE)]))
    ctx.close()
    assert t.nrows == len(strings) and t.columns[0].valid is None
    return t.columns[0].data.view(np.uint64)


def test_converter_bit_exact_against_the_host_parser(converter, tmp_path):
    rng = random.Random(20190101)
    strings = corpus(rng, scale=1)
    assert len(strings) >= 1_000_000
    st, bits = converter(strings)
    assert not (st == REJECT).any(), [s for s, x in zip(strings, st) if x == REJECT][:5]
    want = host_values(strings, tmp_path)
    ok = st == OK
    bad = np.nonzero(ok & (bits != want))[0]
    assert bad.size == 0, [(strings[i], hex(int(bits[i])), hex(int(want[i]))) for i in bad[:5]]
    # undecided: exactly the hexadecimal literals and the decimals of more than 19 significant digits
    for s, x in zip(strings, st):
        if undecidable(s):
            assert x == UNDECIDED, s
        elif x != OK:
            pytest.fail(f"{s!r} left undecided")
    # NaN is the canonical quiet NaN whatever its sign
    nan_bits = {int(b) for s, b in zip(strings, bits) if s.strip().lstrip("+-") == "NaN"}
    assert nan_bits == {0x7FF8000000000000}


def test_converter_rejects_what_java_rejects(converter, tmp_path):
    from queryengine_amd import engine as E
    from queryengine_amd.csv_table import read_csv_native
    bad = ["", " ", "\t", "abc", "1_0", "inf", "nan", "1e", "0x10", "1,5", "--1", "+-1", "1..2", ".", "e5", ".e5", "1e+",
           "0x", "0xp1", "0x1p", "0x1.8", "NaNd", "Infinityf", "infinity", "NAN", "1d5", "1ee5", "1 5", "1.5 x", "½",
           "1.0L", "1e5.5", "0b101", "1f1", "x1", "1-", "+", "-", "d", "1dd"]
    good = [" 2.5e1 ", "7d", "0x1p3", ".5", "5.", "+1E2f", "NaN", "-Infinity", " 0x1.8p1 ", "7D", "-NaN", "1e400",
            "100.5", "25", "8.0", "1e-3", "+.5", "Infinity"]
    st, _ = converter(bad + good)
    ctx = E.Context(device=None, jit_cache_dir=str(tmp_path / "jit"))
    for s, x in zip(bad + good, st):
        try:
            java_parse_double(s)
            python_ok = True
        except NumberFormatException:
            python_ok = False
        if s.strip(" \t"):   # the native parser on a quoted field: an empty one would be NULL, not a number
            try:
                read_csv_native(ctx, f'x\n"{s}"\n'.encode("utf-8"), Schema([Field("x", DataType.DOUBLE)]))
                native_ok = True
            except NumberFormatException:
                native_ok = False
            assert native_ok == python_ok, s
        assert (x != REJECT) == python_ok, (s, int(x))
    ctx.close()
