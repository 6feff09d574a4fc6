"""QE_EXEC_PER_NODE at a size where every loop of qe_pernode_kernels.hip takes more than its first trip.

Every grid in that file is capped, so below a few million rows a lane runs each loop body at most once: the 4-pairs-in-flight
loop of k_arith starts at n > 3 * 2^20, the second chunk step of k_cmp / k_cmp_rows at n > 2^21, the second trip of
k_gather_multi's unrolled loop at m > 2^21 and the second grid-stride trip of every elementwise and ballot kernel at n > 2^22.
One size is past all of them: N = 2^22 + 577, odd and no multiple of 64 or 512.  Bit-exact against the CPU oracle (for the
extension functions and IN / LIKE: the oracle on the lowered plan, member_reference.py).

A numeric literal is a DOUBLE, so "an integer column and a literal" is the cast of the column and DOUBLE arithmetic.
"""
import numpy as np
import pytest

from queryengine_amd import BooleanLiteralExpression, Column, StringLiteralExpression
from queryengine_amd import engine as E
from queryengine_amd import native as N

from expr_lowering import nfn
from helpers import B, D, I32, I64, S, Fn, assert_columns_equal, col, fn, num, random_column
from member_reference import expected_filter_project, in_, like
from test_gpu_parity import run_both

pytestmark = pytest.mark.gpu

ROWS = 2 ** 22 + 577
CMPS = (Fn.CMP_LT, Fn.CMP_LE, Fn.CMP_GE, Fn.CMP_GT, Fn.CMP_EQ, Fn.CMP_NE)
ARITH = (Fn.ADD, Fn.SUB, Fn.MUL, Fn.DIV, Fn.MOD)
DICT = ["k%04d" % i for i in range(16)]
DICT2 = ["k%04d" % i for i in range(8, 28)]       # overlaps DICT: a union remaps the second side's codes

L, M, I, J, X, Y = col("l", 0, I64), col("m", 1, I64), col("i", 2, I32), col("j", 3, I32), col("x", 4, D), col("y", 5, D)
P, Q, S1, S2 = col("p", 6, B), col("q", 7, B), col("s", 8, S), col("t", 9, S)


def lit(s):
    return StringLiteralExpression(s)


_cache = {}


def unfiltered_columns():
    """l INT64, m INT64 in -3 .. 3 (zeros for DIV / MOD), i INT32, j INT32 in -3 .. 3, x DOUBLE with ~20 % NULLs, y DOUBLE with
    specials, p / q BOOLEAN with NULLs, s / t STRING over two small dictionaries (s with NULLs).  Made once, never changed."""
    if "cols" not in _cache:
        rng = np.random.default_rng(2022)
        _cache["cols"] = [random_column(rng, I64, ROWS), Column(I64, rng.integers(-3, 4, ROWS, dtype=np.int64)),
                          random_column(rng, I32, ROWS), Column(I32, rng.integers(-3, 4, ROWS, dtype=np.int32)),
                          random_column(rng, D, ROWS, null_frac=0.2, special=False), random_column(rng, D, ROWS),
                          random_column(rng, B, ROWS, null_frac=0.2), random_column(rng, B, ROWS, null_frac=0.2),
                          random_column(rng, S, ROWS, null_frac=0.1, dictionary=DICT),
                          random_column(rng, S, ROWS, dictionary=DICT2)]
    return _cache["cols"]


def run_lowered(ctx, oracle, cols, flt, projs):
    """run_both for a plan that holds an extension function or IN / LIKE: the expectation is the oracle on the lowered plan."""
    want = expected_filter_project(oracle, cols, flt, projs)
    batch = E.DeviceBatch.from_columns(ctx, cols)
    res = E.filter_project(ctx, batch, ctx.compile(flt) if flt is not None else None, [ctx.compile(p) for p in projs])
    try:
        got = res.to_columns()
        assert res.count == len(want[0])
        for k, (g, w) in enumerate(zip(got, want)):
            assert_columns_equal(g, w, f"projection {k}")
    finally:
        res.free()
        batch.free()
    return got


def test_arithmetic_unary_and_casts(gpu_ctx_per_node, oracle):
    """k_arith in its three types with column operands (integer DIV / MOD over a divisor with zeros: nonzero), DOUBLE with a
    literal operand on either side; unary minus in the three types; the three casts; a numeric literal alone (fill)."""
    cols = unfiltered_columns()
    projs = [fn(f, L, M) for f in ARITH] + [fn(f, I, J) for f in ARITH] + [fn(f, X, Y) for f in ARITH]
    run_both(gpu_ctx_per_node, oracle, cols, None, projs)
    projs = [fn(Fn.MUL, Y, num(2.5)), fn(Fn.SUB, num(1.0), X), fn(Fn.ADD, L, num(7)), fn(Fn.MUL, I, num(3)),
             fn(Fn.UNARY_MINUS, L), fn(Fn.UNARY_MINUS, I), fn(Fn.UNARY_MINUS, Y),
             fn(Fn.ADD, I, L), fn(Fn.ADD, L, X), fn(Fn.ADD, I, Y), num(2.5)]
    got = run_both(gpu_ctx_per_node, oracle, cols, None, projs)
    assert got[7].type == I64 and got[8].type == D and len(got[10]) == ROWS


@pytest.mark.parametrize("mode_name", ["total", "ieee"])
def test_f64_comparisons_in_both_semantics(gpu_ctx_per_node, oracle, mode_name):
    """k_cmp on DOUBLE: six comparisons of a nullable column with one full of NaN, -0.0 and infinities, and with a literal."""
    cols = unfiltered_columns()
    projs = [fn(f, X, Y) for f in CMPS] + [fn(f, Y, num(0.0)) for f in CMPS]
    if mode_name == "total":
        run_both(gpu_ctx_per_node, oracle, cols, None, projs, oracle.BYTECODE_COMPILER)
        return
    gpu_ctx_per_node.set_cmp_semantics(N.CMP_IEEE)
    try:
        run_both(gpu_ctx_per_node, oracle, cols, None, projs, oracle.CLOSURE_COMPILER)
    finally:
        gpu_ctx_per_node.set_cmp_semantics(N.CMP_TOTAL_ORDER)


def test_integer_and_dictionary_comparisons(gpu_ctx_per_node, oracle):
    """k_cmp on INT64; k_cmp_rows (a row per lane) on INT32 and on dictionary codes: = / <> on the codes, the orderings on
    ranks (lookup_codes).  An INT64 and an INT32 column against an integral literal are compared on the integers."""
    cols = unfiltered_columns()
    projs = [fn(f, L, M) for f in CMPS] + [fn(f, I, J) for f in CMPS] + [fn(f, S1, lit("k0007")) for f in CMPS]
    projs += [fn(Fn.CMP_LT, L, num(100)), fn(Fn.CMP_GE, I, num(7)), fn(Fn.CMP_LT, S1, S2)]
    run_both(gpu_ctx_per_node, oracle, cols, None, projs)


def test_logic_and_select(gpu_ctx_per_node, oracle):
    """NOT / AND / OR over nullable BOOLEAN columns (word_not, kleene); IF on a value type, on BOOLEAN (select_words) and on
    STRING across two dictionaries (lookup_codes remaps the second side); a BOOLEAN literal (word_fill)."""
    cols = unfiltered_columns()
    projs = [fn(Fn.NOT, P), fn(Fn.AND, P, Q), fn(Fn.OR, P, Q), fn(Fn.AND, P, fn(Fn.CMP_LT, X, num(0.0))),
             fn(Fn.IF, P, X, Y), fn(Fn.IF, Q, L, M), fn(Fn.IF, P, I, J), fn(Fn.IF, P, Q, fn(Fn.NOT, Q)),
             BooleanLiteralExpression(True)]
    run_both(gpu_ctx_per_node, oracle, cols, None, projs)
    got = run_both(gpu_ctx_per_node, oracle, cols, None, [fn(Fn.IF, Q, S1, S2), lit("lit")])
    assert set(got[0].dictionary) == set(DICT) | set(DICT2) and got[1].dictionary == ["lit"]


def test_null_functions(gpu_ctx_per_node, oracle):
    """ABS in the three types, FLOOR / CEIL; COALESCE on a value type, on BOOLEAN and on STRING (two columns with dictionaries of
    their own, so that the second one's codes are remapped)."""
    cols = unfiltered_columns()
    projs = [nfn(Fn.ABS, L), nfn(Fn.ABS, I), nfn(Fn.ABS, Y), nfn(Fn.FLOOR, Y), nfn(Fn.CEIL, X),
             nfn(Fn.COALESCE, X, Y), nfn(Fn.COALESCE, X, num(-1.0)), nfn(Fn.COALESCE, P, Q), nfn(Fn.COALESCE, S1, S2)]
    run_lowered(gpu_ctx_per_node, oracle, cols, None, projs)


def test_membership(gpu_ctx_per_node, oracle):
    """IN through the bit table (INT64, INT32, dictionary codes) and through the hash set (a wide INT64 list with a member
    beyond 2^53, DOUBLE images with NaN and the two zeros); LIKE."""
    cols = unfiltered_columns()
    narrow = [100 + 3 * k for k in range(33)] + [-7, 7]
    wide = [k * 1000003 - 17000000 for k in range(30)] + [2 ** 53 + 2, -(2 ** 53), 2 ** 31, 99, 101]
    doubles = [k + 0.5 for k in range(30)] + [float("nan"), 0.0, 100.0, float("inf")]
    projs = [in_(L, narrow), in_(I, narrow), in_(S1, DICT[3:9]), in_(L, wide), in_(Y, doubles), like(S1, "k00_1%")]
    got = run_lowered(gpu_ctx_per_node, oracle, cols, None, projs)
    for g in got:                                  # every list has members and non-members among the valid rows
        assert 0 < int(g.data[g.valid if g.valid is not None else slice(None)].sum()) < ROWS


def test_filter_keeping_most_rows(gpu_ctx_per_node, oracle):
    """One conjunct that keeps ~80 % of the rows: more than 3 * 2^20.  `a + b` and `u - v` over non-nullable columns used nowhere
    else read them through the row ids in k_arith's unrolled loop, `c < 10` and `u2 < v2` likewise in k_cmp / k_cmp_rows; the
    nullable x and the BOOLEAN p are gathered (gather_multi, gather_bits_rows) at m > 2^21."""
    rng = np.random.default_rng(2023)
    cols = [Column(D, rng.random(ROWS)), random_column(rng, I64, ROWS), random_column(rng, I64, ROWS),
            Column(D, rng.normal(0, 100, ROWS)), random_column(rng, D, ROWS, null_frac=0.2), random_column(rng, B, ROWS),
            random_column(rng, I32, ROWS), random_column(rng, I32, ROWS), random_column(rng, I32, ROWS),
            random_column(rng, I32, ROWS)]
    F_, A_, B_, C_, X_, P_ = col("f", 0, D), col("a", 1, I64), col("b", 2, I64), col("c", 3, D), col("x", 4, D), col("p", 5, B)
    U_, V_, U2, V2 = col("u", 6, I32), col("v", 7, I32), col("u2", 8, I32), col("v2", 9, I32)
    got = run_both(gpu_ctx_per_node, oracle, cols, fn(Fn.CMP_LT, F_, num(0.8)),
                   [fn(Fn.ADD, A_, B_), fn(Fn.CMP_LT, C_, num(10.0)), X_, P_, fn(Fn.SUB, U_, V_), fn(Fn.CMP_LT, U2, V2)])
    assert 3 * 2 ** 20 < len(got[0]) < ROWS      # run_both has compared this count with the oracle's


def test_filter_narrowing_twice(gpu_ctx_per_node, oracle):
    """The first conjunct keeps ~40 % of the rows, so the domain is narrowed after it; the second is evaluated there (g, x and p
    are gathered for it) and narrows again: narrow() moves the row ids and re-gathers a value column, a nullable one and a
    BOOLEAN bitmap from their compact copies."""
    rng = np.random.default_rng(2024)
    cols = [Column(D, rng.random(ROWS)), Column(D, rng.random(ROWS)), random_column(rng, D, ROWS, null_frac=0.2),
            random_column(rng, B, ROWS), random_column(rng, I64, ROWS)]
    F_, G_, X_, P_, A_ = col("f", 0, D), col("g", 1, D), col("x", 2, D), col("p", 3, B), col("a", 4, I64)
    second = fn(Fn.AND, fn(Fn.CMP_LT, G_, num(0.7)), fn(Fn.OR, fn(Fn.CMP_LT, X_, num(0.0)), P_))
    got = run_both(gpu_ctx_per_node, oracle, cols, fn(Fn.AND, fn(Fn.CMP_LT, F_, num(0.4)), second),
                   [F_, G_, X_, P_, fn(Fn.MUL, A_, A_)])
    assert 0.1 * ROWS < len(got[0]) < 0.4 * ROWS
