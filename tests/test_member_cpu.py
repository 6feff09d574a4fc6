"""IN, LIKE and BETWEEN without a GPU: the expectation's restatements (IN proved equal to the oracle's OR chain of CMP_EQ, LIKE
against hand-written triples), typing and arity through both doors (typecheck.py and qe_expr_compile), the wire format, SQL
text, and the generated source of every route."""
import ctypes as C
import re
import struct

import numpy as np
import pytest

from queryengine_amd import (BooleanLiteralExpression, Column, ColumnExpression, DataType, Function, FunctionExpression,
                             IdentifierExpression, NumericLiteralExpression, SetFunction, StringLiteralExpression)
from queryengine_amd import engine as E
from queryengine_amd import native as N
from queryengine_amd import program, sql, typecheck

from expr_lowering import F64_VECTORS
from helpers import B, D, I32, I64, S, Fn, assert_columns_equal, col, fn, num
from member_reference import expected_filter_project, in_, like, like_matches, literal, np_in, np_like

SetFn = SetFunction
NAN = float("nan")
TWO53 = 2 ** 53


@pytest.fixture(scope="module")
def plan_ctx(native_lib, tmp_path_factory):
    ctx = E.Context(device=None, jit_cache_dir=str(tmp_path_factory.mktemp("jit")))
    yield ctx
    ctx.close()


# ---- the expectation itself -------------------------------------------------------------------------------------------
def _or_chain(x, items):
    e = fn(Fn.CMP_EQ, x, num(items[0]))
    for v in items[1:]:
        e = fn(Fn.OR, e, fn(Fn.CMP_EQ, x, num(v)))
    return e


@pytest.mark.parametrize("mode_name", ["INTERPRETER", "BYTECODE_COMPILER"])
def test_in_restatement_equals_the_oracles_or_chain(oracle, mode_name):
    """x IN (L..) is x = L1 OR .. OR x = Lm by definition: on small lists over hand-written vectors the numpy restatement and
    the oracle's own Kleene OR of CMP_EQ give the same column, NULLs included."""
    mode = getattr(oracle, mode_name)
    cases = [
        (D, F64_VECTORS, [[0.0], [-0.0], [NAN], [-0.0, NAN], [0.5, 2.0 ** 52 + 0.5, float("inf")], [5e-324, -1.5, 0.0]]),
        (I64, [TWO53, -TWO53, TWO53 + 1, TWO53 - 1, -TWO53 - 1, -TWO53 + 1, 0, 1, -(2 ** 63), 2 ** 63 - 1],
         [[float(TWO53)], [float(TWO53 - 1)], [float(TWO53), float(TWO53 - 1)], [-float(TWO53)], [-0.0], [NAN], [0.0, -0.0, NAN],
          [0.5, 1.0], [float(2 ** 63)], [-float(2 ** 63), 1.0]]),
        (I32, [-(2 ** 31), 2 ** 31 - 1, -(2 ** 31) + 1, -1, 0, 1, -7, 7],
         [[-float(2 ** 31)], [float(2 ** 31 - 1), 7.0], [float(2 ** 31)], [-0.0], [NAN, 0.0], [1.5, -7.0]]),
    ]
    for t, vectors, lists in cases:
        n = len(vectors) + 2
        data = np.array(list(vectors) + [vectors[0], vectors[-1]], dtype={D: np.float64, I64: np.int64, I32: np.int32}[t])
        valid = np.ones(n, dtype=bool)
        valid[-2:] = False
        value = Column(t, data, valid)
        x = col("x", 0, t)
        for items in lists:
            want = oracle.filter_project([value], None, [_or_chain(x, items)], mode)[0]
            got = np_in(value, items)
            assert_columns_equal(got, want, f"{t.name} IN {items}")
            assert got.to_list()[-2:] == [None, None]
    # spelled out: 2^53 + 1 converts to 2^53, so it IS in (2^53); -0.0 and NaN match no integer; one NaN, two zeros
    big = Column(I64, np.array([TWO53 + 1, TWO53, TWO53 - 1, 0], dtype=np.int64))
    assert np_in(big, [float(TWO53)]).to_list() == [True, True, False, False]
    assert np_in(big, [float(TWO53 - 1)]).to_list() == [False, False, True, False]
    assert np_in(big, [-0.0, NAN]).to_list() == [False] * 4
    d = Column(D, np.array([0.0, -0.0, NAN, -NAN]))
    assert np_in(d, [-0.0]).to_list() == [False, True, False, False]
    assert np_in(d, [NAN]).to_list() == [False, False, True, True]
    s = Column(S, np.array([0, 1, 2, 7, -3], dtype=np.int32), np.array([True, True, True, False, False]), ["a", "b", "c"])
    assert np_in(s, ["c", "a", "absent"]).to_list() == [True, False, True, None, None]          # garbage codes under the NULLs
    p = Column.from_values(B, [True, False, None])
    assert np_in(p, [True]).to_list() == [True, False, None] and np_in(p, [False]).to_list() == [False, True, None]
    assert np_in(p, [True, False]).to_list() == [True, True, None]


LIKE_TRIPLES = [
    ("", "", True), ("", "a", False), ("a", "", False), ("%", "", True), ("%", "anything", True), ("%%", "", True), ("%%", "xy", True),
    ("_", "", False), ("_", "a", True), ("_", "ab", False), ("_", "\U0001F600", True), ("__", "\U0001F600", False), ("caf_", "café", True),
    ("JFK%", "JFK", True), ("JFK%", "JFK Airport", True), ("JFK%", "LGA JFK", False), ("JFK%", "JF", False),
    ("%port", "Airport", True), ("%port", "ports", False), ("%or%", "Airport", True), ("%or%", "or", True), ("%or%", "o r", False),
    ("a%b%c", "abc", True), ("a%b%c", "a__b__c", True), ("a%b%c", "acb", False), ("a%b", "abab", True), ("a%a", "a", False),
    ("100\\%", "100%", True), ("100\\%", "1000", False), ("a\\_b", "a_b", True), ("a\\_b", "axb", False), ("\\\\", "\\", True),
    ("\\a", "a", True), ("abc", "abc", True), ("abc", "ABC", False), ("abc", "abcd", False), ("%\n%", "a\nb", True), ("a.c", "abc", False),
    ("a_c", "a\nc", True),
]


def test_like_restatement_on_hand_written_triples():
    for pattern, s, want in LIKE_TRIPLES:
        assert like_matches(pattern, s) == want, (pattern, s)
    with pytest.raises(ValueError):
        like_matches("abc\\", "abc")
    c = Column.from_values(S, ["JFK A", None, "LGA", "JFK"])
    assert np_like(c, "JFK%").to_list() == [True, None, False, True]


# ---- typing through both doors ----------------------------------------------------------------------------------------
def _leaf(t, i=0):
    return ColumnExpression(f"c{i}", i, t)


def _both_doors(ctx, raw):
    try:
        py = (typecheck.typeCheck(raw).dataType, None)
    except typecheck.TypeCheckException as e:
        py = (None, str(e))
    try:
        lib = (ctx.compile(raw).result_type, None)
    except Exception as e:   # noqa: BLE001 -- N.check raises the library's message
        lib = (None, str(e))
    if py[1] is None:
        assert lib == py, (raw, py, lib)
    else:
        assert lib[0] is None and py[1] in lib[1], (raw, py, lib)
    return py


def _compile_error(native_lib, ctx, prog):
    h = C.c_void_p()
    st = native_lib.qe_expr_compile(ctx.handle, prog, len(prog), C.byref(h))
    return st, native_lib.qe_last_error(ctx.handle).decode()


def test_typing_rules_through_typecheck_and_the_decoder(plan_ctx):
    F = FunctionExpression
    items = {D: [num(1.0), num(2.5)], S: [literal("a"), literal("b")], B: [literal(True)]}
    numeric = (D, I64, I32)
    for tv in (S, D, B, I64, I32):
        for te, lits in items.items():
            got = _both_doors(plan_ctx, F(SetFn.IN, [_leaf(tv)] + lits))
            if (tv in numeric and te == D) or tv == te:
                assert got == (B, None)
            else:
                assert got == (None, f"Invalid operand types for [IN] [{tv.name}, {te.name}]")
        got = _both_doors(plan_ctx, F(SetFn.LIKE, [_leaf(tv), literal("a%")]))
        assert got == ((B, None) if tv == S else (None, f"Invalid operand types for [LIKE] [{tv.name}, STRING]"))
    # the value is any expression, a literal included
    assert _both_doors(plan_ctx, F(SetFn.IN, [F(Fn.ADD, [_leaf(I64), num(1.0)]), num(3.0)])) == (B, None)
    assert _both_doors(plan_ctx, F(SetFn.IN, [literal("a"), literal("a")])) == (B, None)
    assert _both_doors(plan_ctx, F(SetFn.LIKE, [literal("abc"), literal("a%")])) == (B, None)
    # a pattern that is no literal; a trailing lone backslash
    assert _both_doors(plan_ctx, F(SetFn.LIKE, [_leaf(S, 0), _leaf(S, 1)])) == (None, "Invalid operand types for [LIKE] [STRING, STRING]")
    assert _both_doors(plan_ctx, F(SetFn.LIKE, [_leaf(S), literal("abc\\")])) == (None, "LIKE pattern ends in a lone \\")
    assert _both_doors(plan_ctx, F(SetFn.LIKE, [_leaf(S), literal("abc\\\\")])) == (B, None)
    # typecheck.py: a mixed list, an item that is no literal, too few operands, too many items
    with pytest.raises(typecheck.TypeCheckException, match=r"Invalid operand types for \[IN\] \[DOUBLE, DOUBLE, STRING\]"):
        typecheck.typeCheck(F(SetFn.IN, [_leaf(D), num(1.0), literal("a")]))
    with pytest.raises(typecheck.TypeCheckException, match=r"Invalid operand types for \[IN\] \[DOUBLE, DOUBLE\]"):
        typecheck.typeCheck(F(SetFn.IN, [_leaf(D, 0), _leaf(D, 1)]))
    with pytest.raises(typecheck.TypeCheckException, match=r"\[IN\] expects at least 2 operands, got 1"):
        typecheck.typeCheck(F(SetFn.IN, [_leaf(D)]))
    with pytest.raises(typecheck.TypeCheckException, match=r"\[LIKE\] expects 2 operands, got 3"):
        typecheck.typeCheck(F(SetFn.LIKE, [_leaf(S), literal("a"), literal("b")]))
    with pytest.raises(typecheck.TypeCheckException, match="at most 65536 list items.*SEMI join"):
        typecheck.typeCheck(F(SetFn.IN, [_leaf(D)] + [num(float(i)) for i in range(65537)]))
    assert SetFn.IN.ordinal == 24 and SetFn.LIKE.ordinal == 25 and SetFn.IN.arity == 2 and SetFn.IN.variable_arity and not SetFn.LIKE.variable_arity
    assert SetFn.IN.is_extension and SetFn.LIKE.is_extension and len(Function) == 23                 # Function itself is as it was
    for bad in ([_leaf(D), num(1.0), literal("a")], [_leaf(D), _leaf(D, 1)], [_leaf(D)]):
        with pytest.raises(ValueError):
            program.serialize(F(SetFn.IN, bad))


def test_the_decoder_on_raw_programs(plan_ctx, native_lib):
    """What typecheck.py cannot even express: a list in the wrong place, a bad element type, an empty list, a count above the
    cap, and a list literal cut off at every byte."""
    leaf = program.serialize(_leaf(D))[4:]
    sleaf = program.serialize(_leaf(S))[4:]
    dlist = struct.pack("<BBI", 5, int(D), 2) + struct.pack("<dd", 1.0, 2.0)
    fnb = lambda f: bytes([16, f.ordinal, 0xFF])   # noqa: E731
    H = program.HEADER
    ok = H + leaf + dlist + fnb(SetFn.IN)
    assert ok == program.serialize(FunctionExpression(SetFn.IN, [_leaf(D), num(1.0), num(2.0)]))
    assert _compile_error(native_lib, plan_ctx, ok)[0] == 0
    for prog, msg in (
            (H + dlist + leaf + fnb(SetFn.IN), "Invalid operand types for [IN] [DOUBLE, DOUBLE]"),          # the list first
            (H + dlist + dlist + fnb(SetFn.IN), "Invalid operand types for [IN] [DOUBLE, DOUBLE]"),
            (H + leaf + leaf + fnb(SetFn.IN), "Invalid operand types for [IN] [DOUBLE, DOUBLE]"),           # no list at all
            (H + leaf + dlist + fnb(Fn.ADD), "Invalid operand types for [ADD] [DOUBLE, LIST]"),
            (H + leaf + dlist + fnb(Fn.CMP_EQ), "Invalid operand types for [CMP_EQ] [DOUBLE, LIST]"),
            (H + dlist + fnb(Fn.IS_NULL), "Invalid operand types for [IS_NULL] [LIST]"),
            (H + sleaf + dlist + fnb(SetFn.LIKE), "Invalid operand types for [LIKE] [STRING, LIST]"),
            (H + dlist, "a list literal is only the second operand of IN"),
            (H + leaf + struct.pack("<BBI", 5, int(I64), 1) + struct.pack("<d", 1.0) + fnb(SetFn.IN), "bad list element type"),
            (H + leaf + struct.pack("<BBI", 5, int(D), 0) + fnb(SetFn.IN), "empty list literal"),
            (H + leaf + fnb(SetFn.IN), "stack underflow at IN"),
            (H + leaf + dlist + bytes([16, 26, 0xFF]), "unknown function 26"),
            (H + leaf + dlist + bytes([16, 23, 0xFF]), "unknown function 23")):                                  # 23 is not assigned
        st, err = _compile_error(native_lib, plan_ctx, prog)
        assert st == 2 and msg in err, (prog, st, err)
    # above the cap: QE_ERR_UNSUPPORTED, the message names the SEMI join.  At the cap it compiles.
    st, err = _compile_error(native_lib, plan_ctx, H + leaf + struct.pack("<BBI", 5, int(D), 65537) + fnb(SetFn.IN))
    assert st == 5 and "65536" in err and "SEMI join" in err
    full = H + leaf + struct.pack("<BBI", 5, int(D), 65536) + np.arange(65536, dtype=np.float64).tobytes() + fnb(SetFn.IN)
    assert _compile_error(native_lib, plan_ctx, full)[0] == 0
    # truncated at every byte of the list literal (all three payload kinds)
    slist = struct.pack("<BBI", 5, int(S), 2) + struct.pack("<H", 3) + b"abc" + struct.pack("<H", 0)
    blist = struct.pack("<BBI", 5, int(B), 3) + bytes([1, 0, 1])
    for value, lst in ((leaf, dlist), (sleaf, slist), (program.serialize(_leaf(B))[4:], blist)):
        assert _compile_error(native_lib, plan_ctx, H + value + lst + fnb(SetFn.IN))[0] == 0
        for cut in range(1, len(lst)):
            st, err = _compile_error(native_lib, plan_ctx, H + value + lst[:cut])
            assert st == 2 and "truncated" in err, (cut, st, err)
    assert native_lib.qe_abi_version() == 1 and program.HEADER == b"QEX\x01"


def test_serialised_programs_round_trip_into_the_decoder(plan_ctx):
    a, s, p = _leaf(I64, 0), _leaf(S, 1), _leaf(B, 2)
    tree = typecheck.typeCheck(FunctionExpression(Fn.AND, [
        FunctionExpression(Fn.NOT, [FunctionExpression(SetFn.IN, [a, num(3.0), num(-4.0), num(3.0)])]),
        FunctionExpression(Fn.OR, [FunctionExpression(SetFn.LIKE, [s, literal("J_K%")]),
                                   FunctionExpression(SetFn.IN, [p, literal(True), literal(False)])])]))
    prog = program.serialize(tree)
    assert struct.pack("<BBI", 5, int(D), 3) + struct.pack("<ddd", 3.0, -4.0, 3.0) + bytes([16, 24, int(B)]) in prog
    assert struct.pack("<BBI", 5, int(B), 2) + bytes([1, 0]) + bytes([16, 24, int(B)]) in prog
    assert struct.pack("<BH", 4, 4) + b"J_K%" + bytes([16, 25, int(B)]) in prog
    assert plan_ctx.compile(tree).result_type == B
    u = typecheck.typeCheck(FunctionExpression(SetFn.IN, [s, literal("café"), literal("")]))
    assert struct.pack("<BBI", 5, int(S), 2) + struct.pack("<H", 5) + "café".encode() + struct.pack("<H", 0) in program.serialize(u)
    assert plan_ctx.compile(u).result_type == B


# ---- SQL text ---------------------------------------------------------------------------------------------------------
def test_sql_text():
    ident, F, n = IdentifierExpression, FunctionExpression, NumericLiteralExpression
    pe = sql.parseExpression
    assert pe("a IN (1, -2, +3)") == F(SetFn.IN, [ident("a"), n(1.0), n(-2.0), n(3.0)])                # signed literals fold
    assert pe("v in ('CMT', 'VTS')") == F(SetFn.IN, [ident("v"), literal("CMT"), literal("VTS")])
    assert pe("p IN (TRUE, false)") == F(SetFn.IN, [ident("p"), literal(True), literal(False)])
    assert pe("a NOT IN (1)") == F(Fn.NOT, [F(SetFn.IN, [ident("a"), n(1.0)])])
    # NOT binds tighter than the postfixes, as it does for IS NULL: (NOT a) IN (1), a type error for a numeric a
    assert pe("NOT a IN (1)") == F(SetFn.IN, [F(Fn.NOT, [ident("a")]), n(1.0)])
    with pytest.raises(typecheck.TypeCheckException, match=r"Invalid operand types for \[NOT\] \[DOUBLE\]"):
        typecheck.typeCheck(F(SetFn.IN, [F(Fn.NOT, [_leaf(D)]), n(1.0)]))
    assert pe("a + 1 IN (2) AND p") == F(Fn.AND, [F(SetFn.IN, [F(Fn.ADD, [ident("a"), n(1.0)]), n(2.0)]), ident("p")])
    assert pe("name LIKE 'JFK%'") == F(SetFn.LIKE, [ident("name"), literal("JFK%")])
    assert pe("name NOT LIKE 'it''s\\_%' OR p") == F(Fn.OR, [F(Fn.NOT, [F(SetFn.LIKE, [ident("name"), literal("it's\\_%")])]), ident("p")])
    between = lambda x, lo, hi: F(Fn.AND, [F(Fn.CMP_GE, [x, lo]), F(Fn.CMP_LE, [x, hi])])   # noqa: E731
    assert pe("x BETWEEN 1 AND 2") == between(ident("x"), n(1.0), n(2.0))
    assert pe("x NOT BETWEEN 1 AND 2") == F(Fn.NOT, [between(ident("x"), n(1.0), n(2.0))])
    assert pe("x BETWEEN a - 1 AND b * 2 + 1") == between(ident("x"), F(Fn.SUB, [ident("a"), n(1.0)]),
                                                         F(Fn.ADD, [F(Fn.MUL, [ident("b"), n(2.0)]), n(1.0)]))
    assert pe("x BETWEEN 1 AND 2 AND y") == F(Fn.AND, [between(ident("x"), n(1.0), n(2.0)), ident("y")])
    assert pe("x BETWEEN 1 AND 2 OR y IN (3)") == F(Fn.OR, [between(ident("x"), n(1.0), n(2.0)), F(SetFn.IN, [ident("y"), n(3.0)])])
    # IN, LIKE and BETWEEN stay plain identifiers everywhere else
    assert pe("in + like * between") == F(Fn.ADD, [ident("in"), F(Fn.MUL, [ident("like"), ident("between")])])
    assert pe("IN(a, 1, 2)") == F(SetFn.IN, [ident("a"), n(1.0), n(2.0)])
    q = sql.parseQuery("SELECT a FROM t WHERE zone IN (4, 12, 13) AND name LIKE 'JFK%' ORDER BY 1")
    assert q.filter == F(Fn.AND, [F(SetFn.IN, [ident("zone"), n(4.0), n(12.0), n(13.0)]), F(SetFn.LIKE, [ident("name"), literal("JFK%")])])
    for bad in ("a IN", "a IN ()", "a IN (1", "a IN (b)", "a IN (1 + 2)", "a LIKE", "a LIKE b", "a LIKE 1", "a NOT", "a NOT 1",
                "x BETWEEN 1", "x BETWEEN 1 OR 2", "x BETWEEN 1 AND"):
        with pytest.raises(sql.SyntaxException):
            pe(bad)


# ---- plans ------------------------------------------------------------------------------------------------------------
DICT = ["JFK %d" % i for i in range(30)] + ["LGA %d" % i for i in range(34)]


def _schema_batch(ctx):
    n = 128
    some = np.arange(n) % 3 != 0
    cols = [Column(I64, np.zeros(n, dtype=np.int64)), Column(I64, np.zeros(n, dtype=np.int64)), Column(D, np.zeros(n), some),
            Column(S, np.zeros(n, dtype=np.int32), some, DICT), Column(I32, np.zeros(n, dtype=np.int32), some)]
    return E.DeviceBatch.describe(ctx, cols), (col("a", 0, I64), col("b", 1, I64), col("c", 2, D), col("s", 3, S), col("i", 4, I32))


def _row_text(source):
    """The generated per-row functions (qe_conj<i> / qe_row): where a plan's expressions are."""
    return "\n".join(re.findall(r"qe_(?:conj\d+|row)\(const QeParams &p.*?\n\}", source, re.S))


def test_generated_source_of_every_route(plan_ctx):
    """The thresholds: a chain up to K members (2 <= K <= 32, so 2 is always a chain and 33 never is), a bit table for integers
    of a narrow span, a hash set otherwise.  A table route's text names the route and the slot, never the list."""
    batch, (a, b, c, s, i) = _schema_batch(plan_ctx)
    comp = plan_ctx.compile
    src = lambda flt, projs=(b,): E.generated_source(plan_ctx, batch, comp(flt), [comp(p) for p in projs])   # noqa: E731
    chain = src(in_(a, [7, 1234567]))
    assert "qe_member" not in chain and "== 7ll" in chain and "== 1234567ll" in chain and "(double)" in chain
    bits = src(in_(a, [100 + 3 * k for k in range(33)]))
    assert "qe_member_bits(p, 15, 97ull, " in bits and "qe_member_hash" not in bits
    bits32 = src(in_(i, [100 + 3 * k for k in range(33)]))
    assert "qe_member_bits(p, 15, 97ull, " in bits32
    wide = src(in_(a, [k * 1000003 for k in range(33)]))
    assert "qe_member_hash(p, 15, (u64)(i64)c0)" in wide and "qe_member_bits" not in wide
    dbl = src(in_(c, [k + 0.5 for k in range(33)]))
    assert "qe_member_hash(p, 15, " in dbl and "qe_canon_bits(c0)" in dbl and "qe_member_bits" not in dbl
    big = src(in_(a, [float(TWO53)] + [float(k) for k in range(32)]))                       # |L| >= 2^53: double images of the cast value
    assert "qe_member_hash" in big and "qe_canon_bits(v" in big
    # two 40-literal DOUBLE lists with different values: byte-identical source, one code object
    one = src(in_(c, [k + 0.25 for k in range(40)]))
    two = src(in_(c, [1000.0 * k - 0.75 for k in range(39)] + [NAN]))
    assert one == two and "qe_member_hash" in one
    assert src(in_(a, [k * 1000003 for k in range(40)])) == src(in_(a, [k * 999983 + 5 for k in range(40)]))
    # a plan without IN / LIKE holds neither helper
    plain = src(fn(Fn.CMP_LT, a, num(100)))
    assert "qe_member" not in plain
    # STRING: codes of the dictionary; more than K member codes are a bit table of one bit per code
    sbits = src(in_(s, DICT[10:50] + ["absent"]))
    assert "qe_member_bits(p, 15, 64ull, " in sbits
    one_code = src(in_(s, [DICT[5], "absent"]))
    assert "qe_member" not in one_code and "== 5)" in _row_text(one_code)
    lbits = src(like(s, "LGA%"))
    assert "qe_member_bits(p, 15, 64ull, " in lbits
    assert lbits == src(like(s, "%A _%"))                                                   # 64 entries, >32 members both: same text
    exact = src(like(s, "JFK 7"))                                                           # no wildcard: = against the literal
    assert "qe_member" not in exact and "== 7)" in _row_text(exact)
    # BOOLEAN value
    assert "qe_member" not in src(in_(fn(Fn.CMP_LT, a, num(3)), [True]))


def test_folded_like_reads_the_validity_alone(plan_ctx):
    """A LIKE that matches every entry, or none, loads no table and never reads the column's value: s (slot 0) is read through
    p.colvalid[0] alone, as the direct operand of IS_NULL is."""
    batch, (a, b, c, s, i) = _schema_batch(plan_ctx)
    comp = plan_ctx.compile
    every = E.generated_source(plan_ctx, batch, comp(like(s, "___ %")), [comp(b)])
    assert set(re.findall(r"p\.col\[(\d+)\]", every)) == {"1"} and "p.colvalid[0]" in every and "qe_member" not in every
    assert "alive = (true && kc0);" in every
    none = E.generated_source(plan_ctx, batch, comp(like(s, "EWR%")), [comp(b)])
    assert set(re.findall(r"p\.col\[(\d+)\]", none)) == {"1"} and "qe_member" not in none
    assert "alive = (false && kc0);" in none                                               # the filter keeps nothing
    absent = E.generated_source(plan_ctx, batch, comp(in_(s, ["EWR", "absent"])), [comp(b)])
    assert set(re.findall(r"p\.col\[(\d+)\]", absent)) == {"1"} and "alive = (false && kc0);" in absent
    # projected by value too, the column is loaded again
    also = E.generated_source(plan_ctx, batch, comp(like(s, "___ %")), [comp(b), comp(s)])
    assert set(re.findall(r"p\.col\[(\d+)\]", also)) == {"0", "1"}


def test_plans_of_every_route_compile_without_a_gpu(plan_ctx):
    """hiprtc compiles the kernels: a compile error in the new emitter text or in a helper fails here."""
    batch, (a, b, c, s, i) = _schema_batch(plan_ctx)
    comp = plan_ctx.compile
    flt = fn(Fn.AND, fn(Fn.CMP_LT, a, num(100)), in_(c, [k + 0.5 for k in range(33)]))
    E.prepare(plan_ctx, batch, comp(flt), [comp(in_(a, [100 + 3 * k for k in range(33)])), comp(like(s, "LGA%")),
                                          comp(fn(Fn.NOT, in_(i, [1, 2])))])
    E.prepare_aggregate(plan_ctx, batch, comp(fn(Fn.CMP_LT, a, num(100))),
                        [comp(fn(Fn.IF, in_(s, DICT[10:50]), a, fn(Fn.UNARY_MINUS, a)))], [N.AGG_SUM])
    E.prepare_groupby(plan_ctx, batch, None, [comp(in_(a, [k * 1000003 for k in range(33)])), comp(like(s, "JFK 1%"))],
                      [comp(a)], [N.AGG_SUM])


def test_lowered_expectation(oracle):
    """The walk hands everything but IN / LIKE to the oracle; a value that is an expression is projected by the oracle first."""
    rng = np.random.default_rng(3)
    n = 200
    cols = [Column(I64, rng.integers(0, 50, n, dtype=np.int64), rng.random(n) >= 0.2),
            Column(S, rng.integers(0, 64, n, dtype=np.int32), rng.random(n) >= 0.2, DICT)]
    a, s = col("a", 0, I64), col("s", 1, S)
    flt = fn(Fn.OR, in_(fn(Fn.ADD, a, a), [4, 8, 20]), like(s, "LGA 1%"))
    got = expected_filter_project(oracle, cols, flt, [a, s, fn(Fn.NOT, in_(a, [2, 4]))])
    av, sv = cols[0].to_list(), cols[1].to_list()
    keep = [i for i in range(n) if (av[i] is not None and 2 * av[i] in (4, 8, 20)) or (sv[i] is not None and sv[i].startswith("LGA 1"))]
    assert got[0].to_list() == [av[i] for i in keep] and got[1].to_list() == [sv[i] for i in keep]
    assert got[2].to_list() == [None if av[i] is None else av[i] not in (2, 4) for i in keep]
