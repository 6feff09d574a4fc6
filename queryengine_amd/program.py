"""Expression tree -> postfix program bytes of the C ABI (include/qe_hip.h).

This is the serialiser a Kotlin ``ExpressionVisitor<Unit>`` would implement on
the JVM side: operands first, then the function, so the
library can verify it with a plain operand stack the way the reference's
``MaxStackVisitor`` walks its trees (evaluator/BytecodeCompiler.kt:177-196).
"""
from __future__ import annotations

import struct

from . import ast as A

OP_COLUMN, OP_NUM_LITERAL, OP_BOOL_LITERAL, OP_STR_LITERAL, OP_LIST_LITERAL, OP_FUNCTION = 1, 2, 3, 4, 5, 16
HEADER = b"QEX\x01"


class _Serializer(A.ExpressionVisitor):
    def __init__(self):
        self.out = bytearray(HEADER)

    def visitIdentifier(self, expr):
        raise RuntimeError("Identifier not expected during evaluation")   # Interpreter.kt:9-11

    def visitNumericLiteral(self, expr):
        self.out += struct.pack("<Bd", OP_NUM_LITERAL, float(expr.value))

    def visitBooleanLiteral(self, expr):
        self.out += struct.pack("<BB", OP_BOOL_LITERAL, 1 if expr.value else 0)

    def visitStringLiteral(self, expr):
        b = expr.value.encode("utf-8")
        if len(b) > 0xFFFF:
            raise ValueError("string literal too long")
        self.out += struct.pack("<BH", OP_STR_LITERAL, len(b)) + b

    def visitColumn(self, expr):
        self.out += struct.pack("<BBH", OP_COLUMN, int(expr.dataType), expr.index)

    def list_literal(self, items):
        """u8 op, u8 elem_type, u32 count, then the payloads of the literals without their own opcodes."""
        kinds = {type(o) for o in items}
        if len(kinds) != 1 or not issubclass(next(iter(kinds)), (A.NumericLiteralExpression, A.StringLiteralExpression,
                                                                 A.BooleanLiteralExpression)):
            raise ValueError("the list of IN holds literals of one kind")
        self.out += struct.pack("<BBI", OP_LIST_LITERAL, int(items[0].dataType), len(items))
        for o in items:
            if isinstance(o, A.NumericLiteralExpression):
                self.out += struct.pack("<d", float(o.value))
            elif isinstance(o, A.BooleanLiteralExpression):
                self.out += struct.pack("<B", 1 if o.value else 0)
            else:
                b = o.value.encode("utf-8")
                if len(b) > 0xFFFF:
                    raise ValueError("string literal too long")
                self.out += struct.pack("<H", len(b)) + b

    def visitFunction(self, expr):
        t = 0xFF if expr.dataTypeNullable is None else int(expr.dataTypeNullable)
        if expr.function == A.SetFunction.IN:   # the value, ONE list literal built from the literal operands, the function
            if len(expr.operands) < 2:
                raise ValueError("IN needs a value and at least one literal")
            expr.operands[0].accept(self)
            self.list_literal(expr.operands[1:])
            self.out += struct.pack("<BBB", OP_FUNCTION, expr.function.ordinal, t)
            return
        for op in expr.operands:
            op.accept(self)
        self.out += struct.pack("<BBB", OP_FUNCTION, expr.function.ordinal, t)

    def visitAggregationFunction(self, expr):
        raise RuntimeError("Unexpected aggregation expression in expression compiler")   # Interpreter.kt:111-113


def serialize(expr: A.Expression) -> bytes:
    s = _Serializer()
    expr.accept(s)
    return bytes(s.out)
