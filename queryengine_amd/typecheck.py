"""Type assignment for function nodes -- the host-side twin of the checks libqe_hip repeats
when it verifies a program.

Follows ``evaluator/TypeCheck.kt:38-133`` with four deliberate differences:
  * AND/OR require BOTH operands BOOLEAN (TypeCheck.kt:79-85 demands operands[0] == DOUBLE: a bug
    that makes every ``p AND q`` fail);
  * unary operators check one operand (TypeCheck.kt:50-52 indexes operands[1]);
  * numeric = {DOUBLE, INT64, INT32} with Java binary numeric promotion (extension types);
  * the extension functions IS_NULL / IS_NOT_NULL (any type -> BOOLEAN), COALESCE (typed as IF's branches),
    ABS / FLOOR / CEIL (numeric -> the operand's type), IN (a value and at least one literal, all literals of one kind, the
    value typed against that kind as CMP_EQ types its operands) and LIKE (a STRING and a STRING literal).
"""
from __future__ import annotations

from .ast import (AggregationFunction, AggregationFunctionExpression, BooleanLiteralExpression, DefaultExpressionVisitor,
                  Expression, Function, FunctionExpression, NumericLiteralExpression, SetFunction, StringLiteralExpression)
from .datatypes import DataType, promote


class TypeCheckException(RuntimeError):
    """evaluator/TypeCheck.kt:8"""


def _invalid(function, operands) -> TypeCheckException:
    return TypeCheckException(f"Invalid operand types for [{function.name}] [{', '.join(o.dataType.name for o in operands)}]")


MAX_LIST_ITEMS = 65536   # the cap of a list literal (include/qe_hip.h)
_LITERALS = (NumericLiteralExpression, StringLiteralExpression, BooleanLiteralExpression)


class _TypeCheckVisitor(DefaultExpressionVisitor):
    def visitFunction(self, expr: FunctionExpression) -> Expression:
        ops = self.visitOperands(expr.operands)
        f = expr.function
        if f.variable_arity:
            if len(ops) < f.arity:
                raise TypeCheckException(f"[{f.name}] expects at least {f.arity} operands, got {len(ops)}")
        elif len(ops) != f.arity:
            raise TypeCheckException(f"[{f.name}] expects {f.arity} operands, got {len(ops)}")
        B = DataType.BOOLEAN
        if f in (Function.UNARY_MINUS, Function.UNARY_PLUS, Function.ABS, Function.FLOOR, Function.CEIL):
            if not ops[0].dataType.is_numeric:
                raise _invalid(f, ops)
            return expr.with_(ops, ops[0].dataType)
        if f in (Function.ADD, Function.SUB, Function.MUL, Function.DIV, Function.MOD):
            t = promote(ops[0].dataType, ops[1].dataType)
            if t is None:
                raise _invalid(f, ops)
            return expr.with_(ops, t)
        if f == Function.NOT:
            if ops[0].dataType != B:
                raise _invalid(f, ops)
            return expr.with_(ops, B)
        if f in (Function.CMP_EQ, Function.CMP_NE):
            if promote(ops[0].dataType, ops[1].dataType) is None and ops[0].dataType != ops[1].dataType:
                raise _invalid(f, ops)
            return expr.with_(ops, B)
        if f in (Function.CMP_LT, Function.CMP_LE, Function.CMP_GE, Function.CMP_GT):
            if promote(ops[0].dataType, ops[1].dataType) is None:   # TypeCheck.kt:70-76: numeric only
                raise _invalid(f, ops)
            return expr.with_(ops, B)
        if f in (Function.AND, Function.OR):
            if ops[0].dataType != B or ops[1].dataType != B:
                raise _invalid(f, ops)
            return expr.with_(ops, B)
        if f == Function.IF:
            if ops[0].dataType != B:
                raise _invalid(f, ops)
            t = promote(ops[1].dataType, ops[2].dataType)
            if t is None:
                if ops[1].dataType != ops[2].dataType:
                    raise _invalid(f, ops)
                t = ops[1].dataType
            return expr.with_(ops, t)
        if f in (Function.IS_NULL, Function.IS_NOT_NULL):   # any operand type; never NULL itself
            return expr.with_(ops, B)
        if f == Function.COALESCE:                           # typed as the two branches of IF
            t = promote(ops[0].dataType, ops[1].dataType)
            if t is None:
                if ops[0].dataType != ops[1].dataType:
                    raise _invalid(f, ops)
                t = ops[0].dataType
            return expr.with_(ops, t)
        if f == SetFunction.IN:
            # [value, literal, ...]: the list is of one literal kind, the value against it as CMP_EQ types its operands.  The
            # message names the value's type and the list's element type (every literal's type when they are mixed).
            items = ops[1:]
            if len(items) > MAX_LIST_ITEMS:
                raise TypeCheckException(f"[IN] takes at most {MAX_LIST_ITEMS} list items, got {len(items)}: use a SEMI join for a larger set")
            if not all(isinstance(o, _LITERALS) for o in items) or len({type(o) for o in items}) != 1:
                raise _invalid(f, ops)
            elem = items[0].dataType
            if promote(ops[0].dataType, elem) is None and ops[0].dataType != elem:
                raise _invalid(f, [ops[0], items[0]])
            return expr.with_(ops, B)
        if f == SetFunction.LIKE:
            if ops[0].dataType != DataType.STRING or not isinstance(ops[1], StringLiteralExpression):
                raise _invalid(f, ops)
            if (len(ops[1].value) - len(ops[1].value.rstrip("\\"))) % 2 == 1:
                raise TypeCheckException("LIKE pattern ends in a lone \\")
            return expr.with_(ops, B)
        raise TypeCheckException(f"unknown function {f}")

    def visitAggregationFunction(self, expr: AggregationFunctionExpression) -> Expression:
        ops = self.visitOperands(expr.operands)
        f = expr.function
        if f in (AggregationFunction.MIN, AggregationFunction.MAX, AggregationFunction.SUM, AggregationFunction.AVG):
            if not ops[0].dataType.is_numeric:
                raise TypeCheckException(f"Invalid operand types for aggregation [{f.name}] [{ops[0].dataType.name}]")
        elif f != AggregationFunction.COUNT:
            raise TypeCheckException(f"aggregation [{f.name}] is not implemented (TODO() in the reference, Accumulators.kt:16-17)")
        return AggregationFunctionExpression(f, ops, DataType.DOUBLE, expr.accumulatorIndex)   # TypeCheck.kt:108-120


def typeCheck(expr: Expression) -> Expression:
    return expr.accept(_TypeCheckVisitor())
