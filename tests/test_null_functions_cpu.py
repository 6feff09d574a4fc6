"""IS_NULL / IS_NOT_NULL / COALESCE / ABS / FLOOR / CEIL without a GPU: the expectation's own restatements, typing through
both doors (typecheck.py and qe_expr_compile), SQL text, plan-time compilation and the validity-only load rule."""
import ctypes as C
import random
import re

import numpy as np
import pytest

from queryengine_amd import (BooleanLiteralExpression, Column, ColumnExpression, DataType, Function, FunctionExpression,
                             IdentifierExpression, NumericLiteralExpression, StringLiteralExpression)
from queryengine_amd import engine as E
from queryengine_amd import native as N
from queryengine_amd import program, sql, typecheck

from expr_lowering import (F64_VECTORS, I32_VECTORS, I64_VECTORS, apply_new_function, lower, nfn, np_abs, np_coalesce,
                           np_floor_ceil, np_is_null)
from helpers import B, D, I32, I64, S, ExprGen, Fn, assert_columns_equal, col, fn, num, random_column

ALL_TYPES = (S, D, B, I64, I32)
NUMERIC = (D, I64, I32)


@pytest.fixture(scope="module")
def plan_ctx(native_lib, tmp_path_factory):
    ctx = E.Context(device=None, jit_cache_dir=str(tmp_path_factory.mktemp("jit")))
    yield ctx
    ctx.close()


# ---- the expectation itself -------------------------------------------------------------------------------------------
def test_lowering_leaves_old_trees_alone(oracle):
    """On trees of the reference's 17 functions `lower` is the identity: same objects, same columns, same results."""
    rng = np.random.default_rng(5)
    n = 300
    schema = [("a", D), ("b", I64), ("c", I32), ("p", B), ("q", B)]
    cols = [random_column(rng, t, n, null_frac=0.2) for _, t in schema]
    for seed in range(6):
        g = ExprGen(random.Random(seed), schema, allow_string=False)
        exprs = [g.boolean(3), g.numeric(3), g.boolean(2)]
        for mode in (oracle.BYTECODE_COMPILER,):   # the mode the GPU contexts mirror (test_gpu_parity.run_both)
            lowered, lcols = lower(exprs, cols, oracle, mode)
            assert all(x is y for x, y in zip(lowered, exprs))
            assert len(lcols) == len(cols) and all(x is y for x, y in zip(lcols, cols))
            want = oracle.filter_project(cols, exprs[0], exprs[1:], mode)
            got = oracle.filter_project(lcols, lowered[0], lowered[1:], mode)
            for w, x in zip(want, got):
                assert_columns_equal(x, w)
    assert lower([None], cols, oracle, oracle.BYTECODE_COMPILER)[0] == [None]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64).tolist()


def test_numpy_restatements_on_hand_written_vectors():
    """Bit patterns, written out by hand (java.lang.Math's documented results)."""
    nan = float("nan")
    got = np_abs(Column(D, np.array([-0.0, nan, -nan, float("-inf"), -1.5, 2.5]))).data
    assert _bits(got) == _bits([0.0, nan, nan, float("inf"), 1.5, 2.5])
    assert _bits(got[1:3]) == [0x7FF8000000000000] * 2                      # only the sign bit is touched
    assert np_abs(Column(I64, np.array([-(2 ** 63), -5, 5, 2 ** 63 - 1], dtype=np.int64))).data.tolist() == \
        [-(2 ** 63), 5, 5, 2 ** 63 - 1]                                      # Math.abs(Long.MIN_VALUE) == Long.MIN_VALUE
    assert np_abs(Column(I32, np.array([-(2 ** 31), -5, 5], dtype=np.int32))).data.tolist() == [-(2 ** 31), 5, 5]
    big = 2.0 ** 52
    x = np.array([-0.5, -0.0, 0.0, 0.5, big + 0.5, big - 0.5, -big + 0.5, -big - 0.5, float("inf"), float("-inf"), nan])
    assert big + 0.5 == big and -big - 0.5 == -big                           # not representable: ties to even
    ceil = np_floor_ceil(Column(D, x), ceil=True).data
    floor = np_floor_ceil(Column(D, x), ceil=False).data
    assert _bits(ceil) == _bits([-0.0, -0.0, 0.0, 1.0, big, big, -big + 1.0, -big, float("inf"), float("-inf"), nan])
    assert _bits(floor) == _bits([-1.0, -0.0, 0.0, 0.0, big, big - 1.0, -big, -big, float("inf"), float("-inf"), nan])
    ints = Column(I64, np.array([-3, 7], dtype=np.int64), np.array([True, False]))
    for c in (np_floor_ceil(ints, True), np_floor_ceil(ints, False)):
        assert c.type == I64 and c.to_list() == [-3, None]
    # the vectors the GPU test feeds hold every value asserted above
    assert {-0.0, 0.5, -0.5, big + 0.5, big - 0.5, float("inf")} <= set(F64_VECTORS) and any(v != v for v in F64_VECTORS)
    assert I64_VECTORS[0] == -(2 ** 63) and I32_VECTORS[0] == -(2 ** 31)
    assert np_abs(Column(I64, np.array(I64_VECTORS, dtype=np.int64))).data[0] == -(2 ** 63)
    # COALESCE over {value, NULL}^2
    a = Column.from_values(D, [1.0, 1.0, None, None])
    b = Column.from_values(D, [2.0, None, 2.0, None])
    assert np_coalesce(a, b, D).to_list() == [1.0, 1.0, 2.0, None]
    ai = Column.from_values(I32, [1, 1, None, None])
    assert np_coalesce(ai, b, D).to_list() == [1.0, 1.0, 2.0, None]
    p = Column.from_values(B, [True, False, None, None])
    q = Column.from_values(B, [False, None, True, None])
    assert np_coalesce(p, q, B).to_list() == [True, False, True, None]
    s = Column.from_values(S, ["x", "y", None, None])
    t = Column.from_values(S, ["z", None, "z", None])
    assert np_coalesce(s, t, S).to_list() == ["x", "y", "z", None]
    # null tests read the validity, never the data
    assert np_is_null(a).to_list() == [False, False, True, True] and np_is_null(a).valid is None
    assert np_is_null(a, negate=True).to_list() == [True, True, False, False]
    assert np_is_null(Column(D, np.array([nan, 1.0]))).to_list() == [False, False]
    assert apply_new_function(Fn.IS_NOT_NULL, [b], B).to_list() == [True, False, True, False]


# ---- typing through both doors ----------------------------------------------------------------------------------------
def _leaf(t, i=0):
    return ColumnExpression(f"c{i}", i, t)


def _both_doors(ctx, f, ops):
    """(result type, None) or (None, message) from typecheck.typeCheck and from qe_expr_compile on a serialised, UNTYPED
    tree; the two must agree."""
    raw = FunctionExpression(f, ops)
    try:
        py = (typecheck.typeCheck(raw).dataType, None)
    except typecheck.TypeCheckException as e:
        py = (None, str(e))
    try:
        ce = ctx.compile(raw)
        lib = (ce.result_type, None)
    except Exception as e:   # noqa: BLE001 -- N.check raises the library's message
        lib = (None, str(e))
    if py[1] is None:
        assert lib == py, (f, ops, py, lib)
    else:
        assert lib[0] is None and py[1] in lib[1], (f, ops, py, lib)
    return py


def test_typing_rules_through_typecheck_and_the_decoder(plan_ctx):
    from queryengine_amd import promote
    for t in ALL_TYPES:
        for f in (Fn.IS_NULL, Fn.IS_NOT_NULL):
            assert _both_doors(plan_ctx, f, [_leaf(t)]) == (B, None)
        for f in (Fn.ABS, Fn.FLOOR, Fn.CEIL):
            got = _both_doors(plan_ctx, f, [_leaf(t)])
            if t in NUMERIC:
                assert got == (t, None)                                   # integers keep their type
            else:
                assert got == (None, f"Invalid operand types for [{f.name}] [{t.name}]")
    for ta in ALL_TYPES:
        for tb in ALL_TYPES:
            got = _both_doors(plan_ctx, Fn.COALESCE, [_leaf(ta, 0), _leaf(tb, 1)])
            p = promote(ta, tb)
            if p is not None:
                assert got == (p, None)
            elif ta == tb:
                assert got == (ta, None)
            else:
                assert got == (None, f"Invalid operand types for [COALESCE] [{ta.name}, {tb.name}]")
    # literals are operands like any other
    assert _both_doors(plan_ctx, Fn.IS_NULL, [num(1.0)]) == (B, None)
    assert _both_doors(plan_ctx, Fn.COALESCE, [_leaf(S), StringLiteralExpression("none")]) == (S, None)
    assert _both_doors(plan_ctx, Fn.COALESCE, [_leaf(I64), num(0.0)]) == (D, None)
    # a declared type that disagrees is refused by the decoder
    with pytest.raises(Exception, match=r"declared type DOUBLE of \[IS_NULL\] does not match inferred BOOLEAN"):
        plan_ctx.compile(FunctionExpression(Fn.IS_NULL, [_leaf(D)], D))


def test_arity_errors(plan_ctx, native_lib):
    for f, arity in ((Fn.IS_NULL, 1), (Fn.IS_NOT_NULL, 1), (Fn.COALESCE, 2), (Fn.ABS, 1), (Fn.FLOOR, 1), (Fn.CEIL, 1)):
        assert f.arity == arity and f.is_extension
        with pytest.raises(typecheck.TypeCheckException, match=rf"\[{f.name}\] expects {arity} operands, got {arity + 1}"):
            typecheck.typeCheck(FunctionExpression(f, [_leaf(D, i) for i in range(arity + 1)]))
        # the decoder pops `arity` operands: too few underflow the stack, too many are left over
        few = program.HEADER + b"".join(program.serialize(_leaf(D))[4:] for _ in range(arity - 1)) + bytes([16, f.ordinal, 0xFF])
        many = program.HEADER + b"".join(program.serialize(_leaf(D))[4:] for _ in range(arity + 1)) + bytes([16, f.ordinal, 0xFF])
        for prog, msg in ((few, f"stack underflow at {f.name}"), (many, "must leave exactly one value")):
            h = C.c_void_p()
            st = native_lib.qe_expr_compile(plan_ctx.handle, prog, len(prog), C.byref(h))
            assert st == 2 and msg in native_lib.qe_last_error(plan_ctx.handle).decode()
    assert [f.ordinal for f in Function][17:] == [17, 18, 19, 20, 21, 22] and not Fn.CMP_NE.is_extension
    # one past the last ordinal is still unknown
    prog = program.serialize(_leaf(D)) + bytes([16, 23, 0xFF])
    h = C.c_void_p()
    assert native_lib.qe_expr_compile(plan_ctx.handle, prog, len(prog), C.byref(h)) == 2
    assert "unknown function 23" in native_lib.qe_last_error(plan_ctx.handle).decode()
    assert native_lib.qe_abi_version() == 1 and program.HEADER == b"QEX\x01"


def test_serialised_programs_round_trip_into_the_decoder(plan_ctx):
    a, c, s = _leaf(I64, 0), _leaf(D, 1), _leaf(S, 2)
    tree = typecheck.typeCheck(FunctionExpression(Fn.AND, [
        FunctionExpression(Fn.IS_NOT_NULL, [FunctionExpression(Fn.DIV, [a, a])]),
        FunctionExpression(Fn.CMP_LT, [FunctionExpression(Fn.COALESCE, [FunctionExpression(Fn.ABS, [a]), FunctionExpression(Fn.FLOOR, [c])]),
                                       num(3.0)])]))
    prog = program.serialize(tree)
    assert bytes([16, 18, int(B)]) in prog and bytes([16, 19, int(D)]) in prog and bytes([16, 20, int(I64)]) in prog
    assert plan_ctx.compile(tree).result_type == B
    assert plan_ctx.compile(typecheck.typeCheck(FunctionExpression(Fn.COALESCE, [s, StringLiteralExpression("none")]))).result_type == S
    assert plan_ctx.compile(typecheck.typeCheck(FunctionExpression(Fn.CEIL, [_leaf(I32)]))).result_type == I32


# ---- SQL text ---------------------------------------------------------------------------------------------------------
def test_sql_text():
    ident = IdentifierExpression
    F = FunctionExpression
    assert sql.parseExpression("c IS NULL") == F(Fn.IS_NULL, [ident("c")])
    assert sql.parseExpression("c is not null") == F(Fn.IS_NOT_NULL, [ident("c")])
    # NOT binds tighter than comparison in this grammar (as in the reference), and IS NULL sits at comparison precedence
    assert sql.parseExpression("NOT c IS NULL") == F(Fn.IS_NULL, [F(Fn.NOT, [ident("c")])])
    assert sql.parseExpression("a + b IS NULL AND p") == F(Fn.AND, [F(Fn.IS_NULL, [F(Fn.ADD, [ident("a"), ident("b")])]), ident("p")])
    assert sql.parseExpression("COALESCE(a, b, c)") == F(Fn.COALESCE, [ident("a"), F(Fn.COALESCE, [ident("b"), ident("c")])])
    assert sql.parseExpression("coalesce(a, 0)") == F(Fn.COALESCE, [ident("a"), NumericLiteralExpression(0.0)])
    assert sql.parseExpression("ABS(-a)") == F(Fn.ABS, [F(Fn.UNARY_MINUS, [ident("a")])])
    assert sql.parseExpression("FLOOR(a) < CEIL(b)") == F(Fn.CMP_LT, [F(Fn.FLOOR, [ident("a")]), F(Fn.CEIL, [ident("b")])])
    assert sql.parseExpression("IS_NULL(a)") == F(Fn.IS_NULL, [ident("a")])
    q = sql.parseQuery("SELECT a FROM t WHERE b IS NULL ORDER BY 1 DESC")
    assert q.filter == F(Fn.IS_NULL, [ident("b")]) and q.orderBy == ((1, True),)
    for bad in ("c IS", "c IS NOT", "c IS NOT 1", "c IS b"):
        with pytest.raises(sql.SyntaxException):
            sql.parseExpression(bad)


# ---- plans ------------------------------------------------------------------------------------------------------------
def _schema_batch(ctx):
    n = 128
    some = np.arange(n) % 3 != 0
    cols = [Column(I64, np.zeros(n, dtype=np.int64)), Column(I64, np.zeros(n, dtype=np.int64)), Column(D, np.zeros(n), some),
            Column(S, np.zeros(n, dtype=np.int32), some, ["x", "y"])]
    return E.DeviceBatch.describe(ctx, cols), (col("a", 0, I64), col("b", 1, I64), col("c", 2, D), col("s", 3, S))


def test_plans_compile_without_a_gpu(plan_ctx):
    """hiprtc compiles the generated kernels of a staged filter with IS_NOT_NULL, a STRING COALESCE group-by key and an
    aggregate over COALESCE -- a compile error in the new emitter text fails here."""
    batch, (a, b, c, s) = _schema_batch(plan_ctx)
    comp = plan_ctx.compile
    flt = fn(Fn.AND, nfn(Fn.IS_NOT_NULL, c), fn(Fn.CMP_LT, a, num(100)))
    E.prepare(plan_ctx, batch, comp(flt), [comp(fn(Fn.ADD, a, b))])
    E.prepare_groupby(plan_ctx, batch, None, [comp(nfn(Fn.COALESCE, s, StringLiteralExpression("none")))],
                      [comp(nfn(Fn.ABS, a))], [N.AGG_SUM])
    E.prepare_aggregate(plan_ctx, batch, comp(fn(Fn.CMP_LT, a, num(100))), [comp(nfn(Fn.COALESCE, c, num(0.0)))], [N.AGG_SUM])


def test_validity_only_column_has_no_value_load(plan_ctx, tmp_path):
    """WHERE IS_NOT_NULL(c) AND a < 100 SELECT a + b, c nullable: c is read through its validity bitmap alone.

    The token: every emitter's loads address the values of kernel slot j as `p.col[j]` and its validity words as
    `p.colvalid[j]` (Emitter::loads; every form, every stage of a staged filter and the stage-0 prefetch go through it).
    Slots are handed out in order of first use, filter first: c is slot 0, a slot 1, b slot 2."""
    _, (a, b, c, s) = _schema_batch(plan_ctx)
    flt = fn(Fn.AND, nfn(Fn.IS_NOT_NULL, c), fn(Fn.CMP_LT, a, num(100)))
    # default (staged, ring + two-pass + local forms in one module), always prefetch, dense, unstaged
    for k, bits in enumerate((0, 4194304, 16384, 2048)):
        ctx = E.Context(device=None, jit_cache_dir=str(tmp_path / str(k)), tuning=[0, 0, 0, 0, 0, bits, 0, 0])
        batch = _schema_batch(ctx)[0]
        comp = ctx.compile
        only = E.generated_source(ctx, batch, comp(flt), [comp(fn(Fn.ADD, a, b))])
        assert set(re.findall(r"p\.col\[(\d+)\]", only)) == {"1", "2"}, "a validity-only column must not have its values loaded"
        assert "p.colvalid[0]" in only
        if bits == 4194304:
            assert "qe_s0_load" in only
        also = E.generated_source(ctx, batch, comp(flt), [comp(fn(Fn.ADD, a, b)), comp(c)])
        assert set(re.findall(r"p\.col\[(\d+)\]", also)) == {"0", "1", "2"} and "p.colvalid[0]" in also
        ctx.close()
    # a non-nullable operand folds to a literal at plan time: that column is not read at all
    batch = _schema_batch(plan_ctx)[0]
    comp = plan_ctx.compile
    lit = E.generated_source(plan_ctx, batch, comp(nfn(Fn.IS_NULL, a)), [comp(b)])
    assert "alive = false;" in lit and "p.col[0]" not in lit and "p.colvalid[0]" not in lit
