"""A small recursive-descent front end for the reference's SQL subset.

The reference parses with ANTLR4 (grammar ``src/main/antlr4/.../Query.g4:1-115``,
builder ``parser/ExpressionAstBuilder.kt:8-132``); antlr4-runtime is not
available here, and the parser is host-side planning outside the hot path
(SURVEY.md section 2 row 21).  This restatement exists to drive the hot path from
SQL text in tests and in bench.py.  It keeps the grammar's precedence, which
follows the order of the alternatives of ``expression`` (Query.g4:27-40):

    unary (- + NOT)  >  * / %  >  + -  >  comparison, IS [NOT] NULL, [NOT] IN / LIKE / BETWEEN  >  AND  >  OR

(note that NOT binds tighter than comparison, as in the reference: ``NOT c IS NULL`` is ``(NOT c) IS NULL``;
the postfix null tests and n-ary ``COALESCE(a, b, c)`` = ``COALESCE(a, COALESCE(b, c))`` are extensions, and so are the
postfixes ``x [NOT] IN (literal, ...)``, ``x [NOT] LIKE 'pattern'`` and ``x [NOT] BETWEEN lo AND hi``; BETWEEN is sugar for
``x >= lo AND x <= hi`` whose bounds are parsed at additive precedence, so its AND is its own), all binary
operators left-associative, case-insensitive keywords, numeric literals always
DOUBLE, unary minus/plus folded into numeric literals
(ExpressionAstBuilder.kt:104-110).
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import List, Optional

from .ast import (AggregationFunction, AggregationFunctionExpression, BooleanLiteralExpression, Expression, Function,
                  FunctionExpression, IdentifierExpression, NumericLiteralExpression, SetFunction, StringLiteralExpression)


class SyntaxException(RuntimeError):
    """parser/ParserHelper.kt:9"""


@dataclass(frozen=True)
class Query:
    """ast/Query.kt:3"""
    select: tuple
    from_: str
    filter: Optional[Expression]
    orderByColumn: Optional[int]          # the first ORDER BY ordinal (1-based), as in the reference
    orderBy: tuple = ()                   # every ORDER BY key: (ordinal, descending)
    limit: Optional[int] = None


_TOKEN = re.compile(r"""
    (?P<ws>[ \t\r\n]+)
  | (?P<decimal>[0-9]+(?:\.[0-9]+|[eE][-+]?[0-9]+))
  | (?P<integer>[0-9]+)
  | (?P<ident>[A-Za-z_][A-Za-z_0-9]*)
  | (?P<quoted>"(?:[^"]|"")*")
  | (?P<string>'(?:[^']|'')*')
  | (?P<op>==|!=|<>|<=|>=|[-+*/%=<>(),])
""", re.X)

_KEYWORDS = {"SELECT", "FROM", "WHERE", "ORDER", "BY", "NOT", "AND", "OR", "IF", "THEN", "ELSE", "END", "TRUE", "FALSE"}
_COMPARISONS = {"=": Function.CMP_EQ, "==": Function.CMP_EQ, "!=": Function.CMP_NE, "<>": Function.CMP_NE,
                "<": Function.CMP_LT, "<=": Function.CMP_LE, ">=": Function.CMP_GE, ">": Function.CMP_GT}


def _tokenize(text: str):
    pos, out = 0, []
    while pos < len(text):
        m = _TOKEN.match(text, pos)
        if not m:
            raise SyntaxException(f"token recognition error at: '{text[pos]}' (position {pos})")
        pos = m.end()
        kind = m.lastgroup
        if kind == "ws":
            continue
        val = m.group(kind)
        if kind == "ident" and val.upper() in _KEYWORDS:
            out.append(("kw", val.upper()))
        else:
            out.append((kind, val))
    out.append(("eof", ""))
    return out


class _Parser:
    def __init__(self, text: str):
        self.toks = _tokenize(text)
        self.i = 0

    def peek(self):
        return self.toks[self.i]

    def take(self):
        t = self.toks[self.i]
        self.i += 1
        return t

    def accept(self, kind, val=None):
        k, v = self.peek()
        if k == kind and (val is None or v == val):
            self.i += 1
            return True
        return False

    def expect(self, kind, val=None):
        k, v = self.peek()
        if not self.accept(kind, val):
            raise SyntaxException(f"expected {val or kind} but found '{v}'")
        return v

    # precedence climbing, lowest first
    def expression(self) -> Expression:
        return self.or_()

    def or_(self):
        left = self.and_()
        while self.accept("kw", "OR"):
            left = FunctionExpression(Function.OR, [left, self.and_()])
        return left

    def and_(self):
        left = self.compare()
        while self.accept("kw", "AND"):
            left = FunctionExpression(Function.AND, [left, self.compare()])
        return left

    def compare(self):
        left = self.add()
        while True:
            k, v = self.peek()
            if k == "op" and v in _COMPARISONS:
                self.take()
                left = FunctionExpression(_COMPARISONS[v], [left, self.add()])
            elif k == "ident" and v.upper() == "IS":
                # postfix x IS [NOT] NULL (an extension; IS and NULL stay plain identifiers everywhere else)
                self.take()
                negated = self.accept("kw", "NOT")
                k, v = self.take()
                if k != "ident" or v.upper() != "NULL":
                    raise SyntaxException(f"expected NULL but found '{v}'")
                left = FunctionExpression(Function.IS_NOT_NULL if negated else Function.IS_NULL, [left])
            elif self.member_word(0) or ((k, v) == ("kw", "NOT") and self.member_word(1)):
                # postfix x [NOT] IN (..) / LIKE '..' / BETWEEN a AND b (extensions; the three words stay plain identifiers
                # everywhere else)
                negated = self.accept("kw", "NOT")
                word = self.take()[1].upper()
                if word == "IN":
                    self.expect("op", "(")
                    items = [self.list_item()]
                    while self.accept("op", ","):
                        items.append(self.list_item())
                    self.expect("op", ")")
                    left = FunctionExpression(SetFunction.IN, [left] + items)
                elif word == "LIKE":
                    k, v = self.take()
                    if k != "string":
                        raise SyntaxException(f"expected a string literal after LIKE but found '{v}'")
                    left = FunctionExpression(SetFunction.LIKE, [left, StringLiteralExpression(v[1:-1].replace("''", "'"))])
                else:
                    lo = self.add()
                    self.expect("kw", "AND")
                    hi = self.add()
                    left = FunctionExpression(Function.AND, [FunctionExpression(Function.CMP_GE, [left, lo]),
                                                             FunctionExpression(Function.CMP_LE, [left, hi])])
                if negated:
                    left = FunctionExpression(Function.NOT, [left])
            else:
                return left

    def member_word(self, ahead: int) -> bool:
        k, v = self.toks[min(self.i + ahead, len(self.toks) - 1)]
        return k == "ident" and v.upper() in ("IN", "LIKE", "BETWEEN")

    def list_item(self) -> Expression:
        """A literal of an IN list; a signed numeric literal folds as everywhere else."""
        e = self.unary()
        if not isinstance(e, (NumericLiteralExpression, StringLiteralExpression, BooleanLiteralExpression)):
            raise SyntaxException("the list of IN holds literals only")
        return e

    def add(self):
        left = self.mul()
        while self.peek() in (("op", "+"), ("op", "-")):
            op = self.take()[1]
            left = FunctionExpression(Function.ADD if op == "+" else Function.SUB, [left, self.mul()])
        return left

    def mul(self):
        left = self.unary()
        while self.peek() in (("op", "*"), ("op", "/"), ("op", "%")):
            op = self.take()[1]
            f = {"*": Function.MUL, "/": Function.DIV, "%": Function.MOD}[op]
            left = FunctionExpression(f, [left, self.unary()])
        return left

    def unary(self):
        k, v = self.peek()
        if (k, v) in (("op", "-"), ("op", "+"), ("kw", "NOT")):
            self.take()
            operand = self.unary()
            f = {"-": Function.UNARY_MINUS, "+": Function.UNARY_PLUS, "NOT": Function.NOT}[v]
            if isinstance(operand, NumericLiteralExpression):      # ExpressionAstBuilder.kt:104-110
                if f == Function.UNARY_MINUS:
                    return NumericLiteralExpression(-operand.value)
                if f == Function.UNARY_PLUS:
                    return operand
            return FunctionExpression(f, [operand])
        return self.primary()

    def primary(self):
        k, v = self.take()
        if k in ("decimal", "integer"):
            return NumericLiteralExpression(float(v))               # :26-28 toDouble()
        if k == "kw" and v in ("TRUE", "FALSE"):
            return BooleanLiteralExpression(v == "TRUE")
        if k == "string":
            return StringLiteralExpression(v[1:-1].replace("''", "'"))
        if k == "kw" and v == "IF":
            c = self.expression(); self.expect("kw", "THEN")
            t = self.expression(); self.expect("kw", "ELSE")
            e = self.expression(); self.expect("kw", "END")
            return FunctionExpression(Function.IF, [c, t, e])
        if k == "op" and v == "(":
            e = self.expression()
            self.expect("op", ")")
            return e
        if k == "ident":
            if self.accept("op", "("):
                ops = [self.expression()]
                while self.accept("op", ","):
                    ops.append(self.expression())
                self.expect("op", ")")
                name = v.upper()
                if name == "COALESCE" and len(ops) > 2:                 # n-ary: folds to the right
                    e = ops[-1]
                    for op in reversed(ops[:-1]):
                        e = FunctionExpression(Function.COALESCE, [op, e])
                    return e
                if name in Function.__members__:
                    return FunctionExpression(Function[name], ops)
                if name in SetFunction.__members__:
                    return FunctionExpression(SetFunction[name], ops)
                if name in AggregationFunction.__members__:
                    return AggregationFunctionExpression(AggregationFunction[name], ops)
                raise SyntaxException(f"Unsupported function {name}")   # :62
            return IdentifierExpression(v)
        if k == "quoted":
            return IdentifierExpression(v[1:-1].replace('""', '"'))
        raise SyntaxException(f"unexpected token '{v}'")

    def identifier(self) -> str:
        k, v = self.take()
        if k == "ident":
            return v
        if k == "quoted":
            return v[1:-1].replace('""', '"')
        raise SyntaxException(f"expected identifier but found '{v}'")


def parseExpression(text: str) -> Expression:
    """parser/ParserHelper.kt:44-46"""
    p = _Parser(text)
    e = p.expression()
    p.expect("eof")
    return e


def parseQuery(text: str) -> Query:
    """parser/ParserHelper.kt:48-57"""
    p = _Parser(text)
    p.expect("kw", "SELECT")
    select = [p.expression()]
    while p.accept("op", ","):
        select.append(p.expression())
    p.expect("kw", "FROM")
    from_ = p.identifier()
    flt = p.expression() if p.accept("kw", "WHERE") else None
    # ORDER BY n [ASC|DESC] {, n [ASC|DESC]} [LIMIT k] (the reference has one ascending ordinal: Query.g4:19).  ASC, DESC
    # and LIMIT are plain identifiers everywhere else: they are only looked for here.
    def word(*names):
        k, v = p.peek()
        if k == "ident" and v.upper() in names:
            p.take()
            return v.upper()
        return None

    keys = []
    limit = None
    if p.accept("kw", "ORDER"):
        p.expect("kw", "BY")
        while True:
            ordinal = int(p.expect("integer"))
            keys.append((ordinal, word("ASC", "DESC") == "DESC"))
            if not p.accept("op", ","):
                break
        if word("LIMIT"):
            limit = int(p.expect("integer"))
    p.expect("eof")
    return Query(tuple(select), from_, flt, keys[0][0] if keys else None, tuple(keys), limit)
