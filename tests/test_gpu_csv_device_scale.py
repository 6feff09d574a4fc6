"""The device CSV parser (qe_csv_device.cpp / .hip, qe_csv_number.h) at the sizes and inputs where its code changes
path: the decimal -> double converter as DEVICE code on the corpus of tests/test_csv_device_cpu.py, the recursive scan at its
third level, the dictionary beyond one workgroup of the scan (2048 entries) and one block of the pack kernel (256), texts of
2047 / 2048 / 2049 tiles and of length 0, 1, 4095 mod 4096 under every kind of last byte, and the patch list: full, one
field past full, and its fields as the shared packer brings them to the host.

Every test compares the device batch with the host parser (qe_csv_parse + qe_csv_pin) through ``check_parity``: bit-equal
data words, validity words, nullability and dictionaries.  Nothing here has a tolerance.  What a test is about (a row count,
a distinct count, a tile count, a number of patched fields) it asserts from its own input."""
import random

import pytest

from csv_number_corpus import corpus, undecidable
from test_gpu_csv_device import B, D, S, check_parity, stats
from queryengine_amd import Field, Schema
from queryengine_amd.csv_table import read_csv_device

pytestmark = pytest.mark.gpu

TILE = 4096                      # kCsvTile: text bytes per wave of the structure passes
SCAN_BLOCK = 1024                # kScanBlock (qe_scan.h): elements per workgroup of exclusive_scan, block sums per trip of its carry scan
SCAN_PER = 2048                  # elements per workgroup of the parser's former recursive scan: its seams stay in the cases
PACK_BLOCK = 256                 # fields per block of dict_pack_kernel: the distinct strings, or the patch list
PATCH_CAP = 1 << 20              # undecided fields of one column that the patch list holds
# scan() works on n + 1 elements (the total lands behind the last): exclusive_scan in workgroups of kScanBlock, whose sums ONE
# workgroup scans in trips of kScanBlock with a carry.  Its second trip begins at n + 1 = 1024 * 1024 + 1.
CARRY_TRIP = SCAN_BLOCK * SCAN_BLOCK
# The former scan recursed instead: its 2048th workgroup, and with it a third level, began at n + 1 = 2047 * 2048 + 1.
THREE_LEVEL = (SCAN_PER - 1) * SCAN_PER


def quoted(s):
    return '"' + s.replace('"', '""') + '"'


def field(s):
    """`s` as a CSV field, enclosed only where it has to be"""
    return quoted(s) if any(c in s for c in ',\n\r"') else s


# ---- 1. the converter on the device ---------------------------------------------------------------------------------------
MAX_HARD = 1000                  # undecidable strings kept: few enough that the test below stays one about the device's converter


@pytest.fixture(scope="module")
def number_strings():
    """(strings, undecidable ones among them): the CPU test's corpus at a fifth of its random draws, every string that the
    CPU test's rule calls decidable, and MAX_HARD of the others (every hexadecimal literal among them)."""
    strings = corpus(random.Random(20190101), scale=0.2)
    hard = [i for i, s in enumerate(strings) if undecidable(s)]
    hexa = [i for i in hard if "x" in strings[i].lower()]
    rest = [i for i in hard if "x" not in strings[i].lower()]
    drop = set(hard) - set(hexa) - set(random.Random(1).sample(rest, MAX_HARD - len(hexa)))
    kept = [s for i, s in enumerate(strings) if i not in drop]
    return kept, [s for s in kept if undecidable(s)]


def test_converter_on_the_device(gpu_ctx, number_strings):
    strings, hard = number_strings
    assert len(hard) == MAX_HARD and any(s.strip().startswith("0x") for s in hard)
    # the condition under which this test is about the device: the host's strtod converts at most 1 % of the rows
    assert len(hard) <= 0.01 * len(strings)
    text = ("x\n" + "\n".join(strings) + "\n").encode("latin-1")
    st = check_parity(gpu_ctx, text, Schema([Field("x", D)]))
    assert st.host_fallback == 0 and st.nrows == len(strings)
    # exactly the strings that may be left to the host: the Eisel-Lemire "ambiguous" exit never fires on this corpus in the
    # host build of the header, and must not on the device
    assert st.host_patched_fields == len(hard)


def test_converter_over_three_columns(gpu_ctx, number_strings):
    strings, hard = number_strings
    rng = random.Random(2)
    easy = [s for s in strings if not undecidable(s)]
    fields = hard + easy[::7]
    rng.shuffle(fields)
    cells = []
    for s in fields:
        if rng.random() < 0.05:
            cells.append("")                                   # NULL
        cells.append(quoted(s) if rng.random() < 0.15 else s)
    cells += [""] * (-len(cells) % 3)
    rows = [cells[i:i + 3] for i in range(0, len(cells), 3)]
    per_column = [sum(1 for r in rows if undecidable(r[k].strip('"')) and r[k]) for k in range(3)]
    # the patch counter starts again for every column, and every column's scatter takes more than one block of 256
    assert sum(per_column) == len(hard) and min(per_column) > 256
    text = ("x,y,z\n" + "".join(",".join(r) + rng.choice(["\n", "\r\n"]) for r in rows)).encode("latin-1")
    st = check_parity(gpu_ctx, text, Schema([Field("x", D), Field("y", D), Field("z", D)]))
    assert st.host_fallback == 0 and st.nrows == len(rows)
    assert st.host_patched_fields == len(hard)


# ---- 2. scan depth -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def key_block():
    """4099 rows `key,flag` over 3000 distinct keys of 1 to 3 characters: the rows of a block, and the same rows in another
    order for the ragged tail"""
    rng = random.Random(3)
    keys = [f"{i:x}" for i in range(3000)]
    keys += rng.sample(keys, 1099)
    rng.shuffle(keys)
    flags = ["true", "false", "TRUE", "", "x", "tRuE", "false"]
    rows = [f"{k},{flags[i % len(flags)]}\n" for i, k in enumerate(keys)]
    return rows, rows[::-1]


@pytest.mark.parametrize("nrows", [CARRY_TRIP - 2, CARRY_TRIP - 1, CARRY_TRIP + SCAN_BLOCK + 1, THREE_LEVEL - 1, THREE_LEVEL, THREE_LEVEL + 2049])
def test_rank_scan_at_its_third_level(gpu_ctx, key_block, nrows):
    """The rank scan of a STRING column runs over the rows: the only scan of the parser that can reach the second trip of the
    carry scan over the block sums (a tile scan would need 4 GiB of text).  The scanned n + 1 elements are one short of a full
    trip, exactly one trip, and one block past it; then the row counts at which the former recursive scan took its third level."""
    rows, other = key_block
    # NULLs in the last 64-row word: of the key, of the flag, of both
    last = [",true\n", "7,\n", ",\n", "a,false\n"] * 16
    reps, ragged = divmod(nrows - len(last), len(rows))
    text = ("k,f\n".encode() + "".join(rows).encode() * reps + "".join(other[:ragged]).encode() + "".join(last).encode())
    st = check_parity(gpu_ctx, text, Schema([Field("k", S), Field("f", B)]))
    assert st.host_fallback == 0 and st.nrows == nrows


# ---- 3. dictionary growth ---------------------------------------------------------------------------------------------------
def dict_text(rng, strings, copies=3, empty=0.05):
    """`k,v` rows: every string `copies` times and a share of empty fields, shuffled"""
    cells = [field(s) for s in strings] * copies
    cells += [""] * int(len(cells) * empty)
    rng.shuffle(cells)
    return ("k,v\n" + "".join(f"{c},{i % 10}\n" for i, c in enumerate(cells))).encode("utf-8"), len(cells)


KV = Schema([Field("k", S), Field("v", D)])


@pytest.mark.parametrize("nd", [PACK_BLOCK - 1, PACK_BLOCK, PACK_BLOCK + 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, SCAN_PER - 1, SCAN_PER, SCAN_PER + 1,
                                5003])
def test_dictionary_sizes(gpu_ctx, nd):
    """nd distinct strings: dict_pack_kernel's second block begins at 257, and the scan over their nd + 1 lengths takes a
    second workgroup from nd = 1024 on (from 2048 on in the former scan).  Every string appears three times in shuffled order, so the order of first appearance
    is neither the sorted order nor the order of the hash table."""
    rng = random.Random(nd)
    strings = [f"k{i}" + "é" * (i % 3) + "x" * (i * 7 % 37) for i in range(nd)]
    assert len(set(strings)) == nd
    text, nrows = dict_text(rng, strings)
    st = check_parity(gpu_ctx, text, KV)
    assert st.host_fallback == 0 and st.nrows == nrows


def test_dictionary_of_distinct_rows(gpu_ctx):
    """A column of timestamps: every row a string of its own, 100 000 entries in the table and in the packed dictionary."""
    n = 100_000
    stamps = [f"2019-01-{1 + i // 3600 % 28:02d} {i // 3600 % 24:02d}:{i // 60 % 60:02d}:{i % 60:02d}.{i * 7919 % 1000000:06d}"
              for i in range(n)]
    assert len(set(stamps)) == n
    text, nrows = dict_text(random.Random(4), stamps, copies=1, empty=0)
    st = check_parity(gpu_ctx, text, KV)
    assert st.host_fallback == 0 and st.nrows == nrows == n


def unescaped(cell):
    return cell[1:-1].replace('""', '"') if cell.startswith('"') else cell


def expected_dictionary(cells):
    out = []
    for c in cells:
        s = unescaped(c)
        if s and s not in out:
            out.append(s)
    return out


def test_one_string_written_in_several_ways(gpu_ctx):
    """Entries are equal when their UNESCAPED bytes are: same_string on fields of different raw lengths."""
    pool = ['ab', '"ab"', '"a""b"', '"a""b"', '""""', '""""""', '"""ab"', '"ab"""', '"a""""b"', '"x,""y"""', '"x,""y"""',
            'abcdefg1', 'abcdefg2', '"abcdefg1"', '"abcdefg3"', 'abc', 'abcd', '"abc"', '"a,b"', '"a,c"',
            '"ab,"', 'ab ', ' ab', '"a\nb"', '"a\r\nb"', '""', '']
    rng = random.Random(5)
    cells = pool + [rng.choice(pool) for _ in range(3000)]
    text = ("k,v\n" + "".join(f"{c},{i % 10}\n" for i, c in enumerate(cells))).encode()
    st = check_parity(gpu_ctx, text, KV)
    assert st.host_fallback == 0 and st.nrows == len(cells)
    want = expected_dictionary(cells)
    assert want[:5] == ['ab', 'a"b', '"', '""', '"ab'] and len(want) == len(set(want))
    dev = read_csv_device(gpu_ctx, text, KV)
    assert stats(gpu_ctx).host_fallback == 0
    assert dev.dictionaries[0] == want
    dev.batch.free()


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 1500])
def test_long_quoted_fields(gpu_ctx, shift):
    """Three enclosed fields of about 10 KB, each across more than two tiles, with line ends, commas and "" escapes inside:
    two are equal, the third differs from them in its last byte only, and other rows stand between them."""
    piece = 'line one\nline "two"\r\n3,4,5\r""x"",\n'
    body = piece * (10_000 // len(piece))
    assert len(quoted(body + "A")) > 2 * TILE
    small = [f"s{i},{i}.5\n" for i in range(40)]
    cells = [body + "A", body + "A", body + "B"]
    text = ("k,v\n" + "p" * shift + ",0\n" + "".join(small[:7]) + quoted(cells[0]) + ",1\r\n" + "".join(small[7:30])
            + quoted(cells[1]) + ",2\n" + "".join(small[30:]) + quoted(cells[2]) + ",3\n" + "s1,9\n").encode()
    st = check_parity(gpu_ctx, text, KV)
    assert st.host_fallback == 0 and st.nrows == 45
    dev = read_csv_device(gpu_ctx, text, KV)
    names = [f"s{i}" for i in range(40)]
    want = (["p" * shift] if shift else []) + names[:7] + [cells[0]] + names[7:] + [cells[2]]
    assert dev.dictionaries[0] == want
    dev.batch.free()


# ---- 4. tile arithmetic ----------------------------------------------------------------------------------------------------
# the last bytes of the text; the header is `b,a`, so the STRING field stands last
ENDINGS = {"closing quote": '2.5,"q,\r\n"',
           "lone CR": "2.5,q\r",
           "CR LF": "2.5,q\r\n",
           "no line end": "2.5,q",
           "escaped pair, then the closing quote": '2.5,"q"""'}
# padding: unquoted STRING fields (a long digit run would go to the patch list), 64 rows of 50 to 80 bytes
PAD = "".join(f"{k * 1.5},pad{k % 7}{'x' * (40 + k % 29)}\n" for k in range(64))
BA = Schema([Field("a", S), Field("b", D)])


def tile_text(n, ending):
    """(`b,a` and a body of exactly n bytes that ends in `ending`, its rows): tiles are counted from the body's first byte"""
    room = n - len(ending)
    reps = max(0, room - 300) // len(PAD)
    fill = room - reps * len(PAD)                  # 300 .. 300 + len(PAD) bytes: one row that makes the length exact
    assert fill >= 6
    body = PAD * reps + "7.5," + "y" * (fill - 5) + "\n" + ending
    assert len(body) == n
    return ("b,a\n" + body).encode(), 64 * reps + 2


def tile_lengths(ntiles):
    """the lengths 1, 4095 and 0 mod 4096 that make `ntiles` tiles"""
    return [(ntiles - 1) * TILE + 1, ntiles * TILE - 1, ntiles * TILE]


@pytest.mark.parametrize("ntiles", [1, 2, 3, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, SCAN_PER - 1, SCAN_PER, SCAN_PER + 1])
def test_tile_counts_lengths_and_last_bytes(gpu_ctx, ntiles):
    """1023 tiles (+ 1 for the total) are the last that one workgroup of the tile scans holds (2047 in the former scan).  At a length of 0 or 1 mod 4096
    the text's last byte is the last or the only byte of its tile, and when that byte is a closing quote, a lone \\r or the \\n
    of a \\r\\n, the end-of-text and carried-byte branches of records_kernel decide alone."""
    for n in tile_lengths(ntiles) if ntiles > 1 else [TILE - 1, TILE]:   # (no ending fits a body of one byte)
        assert (n + TILE - 1) // TILE == ntiles
        for what, ending in ENDINGS.items():
            text, nrows = tile_text(n, ending)
            st = check_parity(gpu_ctx, text, BA)
            assert st.host_fallback == 0 and st.text_bytes == len(text) and st.nrows == nrows, (n, what)


MIB = 1 << 20


@pytest.mark.parametrize("n, threads", [(8 * MIB + 1, 2), (12 * MIB + 2, 3), (36 * MIB + 7, 8)])
def test_text_lengths_that_do_not_divide_among_the_fill_threads(gpu_ctx, tmp_path, n, threads):
    """A chunk of at least 8 MiB is staged by n / 4 MiB (at most 8) threads, a whole number of 4 KiB pages each.  Here the
    n / threads bytes of one thread are whole pages already and n % threads bytes remain: they are the last thread's too.
    (They once were nobody's, and the text's last bytes reached the device as whatever the staging buffer held: the first
    text of 2049 tiles found it.)  Two texts of one length that differ in their last bytes, so that what the first leaves
    in the staging buffer is not what the second needs; from bytes and from a file."""
    assert min(8, n // (4 * MIB)) == threads and n // threads % 4096 == 0 and n % threads != 0
    for k, ending in enumerate(("2.5,ABCDEFGH", "2.5,stuvwxyz")):
        text, nrows = tile_text(n, ending)
        p = tmp_path / f"split{k}.csv"
        p.write_bytes(text)
        for src in (text, str(p)):
            st = check_parity(gpu_ctx, src, BA)
            assert st.host_fallback == 0 and st.text_bytes == len(text) and st.nrows == nrows


# ---- 5. patch overflow -----------------------------------------------------------------------------------------------------
def test_patch_list_overflow_falls_back(gpu_ctx):
    """One undecided field more than the patch list holds: the whole input goes to the host, and the context is good for the
    next parse."""
    lits = ["0x1p3", "0x1.8p1", "-0x1.fffffffffffffp1023", "0X.8P-1d", "0x1p-1074", "0xAp0", " 0x.1p+4 "]
    n = PATCH_CAP + 1
    rows = (lits * (n // len(lits) + 1))[:n]
    text = ("x\n" + "\n".join(rows) + "\n").encode()
    sch = Schema([Field("x", D)])
    st = check_parity(gpu_ctx, text, sch, fallback=1)
    assert st.host_fallback == 1 and st.nrows == n
    st = check_parity(gpu_ctx, b"x\n0x1p3\n1.5\n\n2e400\n", sch)
    assert st.host_fallback == 0 and st.host_patched_fields == 1 and st.nrows == 3


def test_patch_list_exactly_full(gpu_ctx):
    """PATCH_CAP undecided fields, the most the device path patches.  Row i is the hexadecimal literal of i: every value is
    distinct and the lengths run from 1 to 5 digits, so a wrong offset, slice or scatter slot is a wrong value."""
    n = PATCH_CAP
    text = ("x\n" + "".join(f"0x{i:x}p0\n" for i in range(n))).encode()
    st = check_parity(gpu_ctx, text, Schema([Field("x", D)]))
    assert st.host_fallback == 0 and st.host_patched_fields == n and st.nrows == n


def test_patched_fields_written_in_several_ways(gpu_ctx):
    """One column whose undecidable fields are plain, enclosed, and enclosed with spaces around the literal: the packer hands
    the host the content without the quotes, in the order of the patch list, which is not the row order.  Decidable rows
    stand between them.  More than one block of the length and pack kernels."""
    hard = ["0x1p3", '"0x1p3"', '" 0x1p3 "', "123456789012345678901234567", '"123456789012345678901234567"',
            '" 123456789012345678901234567 "']
    cells = []
    for i in range(700):
        cells += [hard[i % len(hard)] if i % 5 else f'"0x{i:x}p-{i % 9}"', "1e3", '""', f"{i}.25"][: 2 + i % 3]   # ("": NULL)
    nhard = sum(1 for c in cells if "x" in c or len(c) > 20)
    assert nhard == 700 > 2 * PACK_BLOCK and len(cells) > 2 * nhard
    text = ("x\n" + "".join(c + "\n" for c in cells) + "0x1p3").encode()
    st = check_parity(gpu_ctx, text, Schema([Field("x", D)]))
    assert st.host_fallback == 0 and st.host_patched_fields == nhard + 1 and st.nrows == len(cells) + 1
