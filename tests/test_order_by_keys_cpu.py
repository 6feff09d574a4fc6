"""ORDER BY several columns, ASC / DESC, LIMIT: grammar, logical plan, the host branch of OrderByOperator and the ABI
declaration (no GPU).  The order is Kotlin's ``compareBy().thenByDescending()`` on a stable ``sortWith``."""
import functools
import itertools
import os
import re

import pytest

from queryengine_amd import Column, ColumnarTable, DataType, Field, Schema, TableRegistry
from queryengine_amd import native as N
from queryengine_amd.operators import Operator, OrderByOperator, _compare_key, map as op_map
from queryengine_amd.planner import (LogicalAggregationNode, LogicalFilterNode, LogicalOrderByNode, LogicalProjectionNode,
                                     buildLogicalPlan)
from queryengine_amd.sql import Query, SyntaxException, parseQuery

D, I64, B, S = DataType.DOUBLE, DataType.INT64, DataType.BOOLEAN, DataType.STRING
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Rows(Operator):
    def __init__(self, rows):
        self.rows, self.i = rows, None

    def open(self):
        self.i = 0

    def close(self):
        self.i = None

    def next(self):
        if self.i >= len(self.rows):
            return None
        self.i += 1
        return self.rows[self.i - 1]


def test_parse_order_by_keys_and_limit():
    q = parseQuery("SELECT a + b, c FROM t WHERE a < 100 ORDER BY 2 DESC, 1 LIMIT 10")
    assert q.orderBy == ((2, True), (1, False)) and q.limit == 10 and q.orderByColumn == 2
    q = parseQuery("SELECT a, c FROM t ORDER BY 2")
    assert q.orderByColumn == 2 and q.orderBy == ((2, False),) and q.limit is None
    q = parseQuery("select a, c from t order by 1 asc, 2 desc limit 0")
    assert q.orderBy == ((1, False), (2, True)) and q.limit == 0
    q = parseQuery("SELECT a FROM t")
    assert q.orderByColumn is None and q.orderBy == () and q.limit is None
    assert Query(q.select, "t", None, None) == q                    # four-argument construction still works


def test_asc_desc_limit_are_not_reserved_words():
    q = parseQuery("SELECT limit, desc FROM t ORDER BY 1")
    assert [e.name for e in q.select] == ["limit", "desc"] and q.orderBy == ((1, False),)
    q = parseQuery("SELECT asc + limit FROM limit WHERE desc < 1 ORDER BY 1 DESC LIMIT 2")
    assert q.from_ == "limit" and q.orderBy == ((1, True),) and q.limit == 2


@pytest.mark.parametrize("sql", ["SELECT a FROM t LIMIT 5", "SELECT a FROM t WHERE a < 1 LIMIT 5", "SELECT a FROM t ORDER BY 1 LIMIT -1",
                                 "SELECT a FROM t ORDER BY 1 DESC DESC", "SELECT a FROM t ORDER BY 1 LIMIT", "SELECT a FROM t ORDER BY 1,",
                                 "SELECT a FROM t ORDER BY DESC", "SELECT a FROM t ORDER BY 1 LIMIT 2 LIMIT 3", "SELECT a FROM t ORDER BY 1 LIMIT 1.5"])
def test_order_by_parse_errors(sql):
    with pytest.raises(SyntaxException):
        parseQuery(sql)


def _registry():
    schema = Schema([Field("a", D), Field("b", D), Field("c", D), Field("s", S)])
    r = TableRegistry()
    r.register("t", ColumnarTable.from_rows(schema, [[1.0, 2.0, 0.5, "x"]]))
    return r


def test_logical_plan_carries_keys_and_limit():
    r = _registry()
    plain = buildLogicalPlan(r, parseQuery("SELECT a + b, c FROM t WHERE a < 100"))      # (plans compare by their repr:
    # two separately built expression trees are not == each other)
    ordered = buildLogicalPlan(r, parseQuery("SELECT a + b, c FROM t WHERE a < 100 ORDER BY 2 DESC, 1 LIMIT 10"))
    assert isinstance(ordered, LogicalOrderByNode) and ordered.index == 2
    assert ordered.keys == ((2, True), (1, False)) and ordered.limit == 10
    assert repr(ordered.source) == repr(plain) and isinstance(plain, LogicalProjectionNode) and isinstance(plain.source, LogicalFilterNode)
    single = buildLogicalPlan(r, parseQuery("SELECT a + b, c FROM t WHERE a < 100 ORDER BY 2"))
    assert single.index == 2 and single.limit is None and repr(single.source) == repr(plain)
    top = buildLogicalPlan(r, parseQuery("SELECT s, SUM(a) FROM t ORDER BY 2 DESC LIMIT 3"))
    assert top.keys == ((2, True),) and top.limit == 3 and top.index == 2
    assert repr(top.source) == repr(buildLogicalPlan(r, parseQuery("SELECT s, SUM(a) FROM t")))
    assert isinstance(top.source.source, LogicalAggregationNode)
    assert LogicalOrderByNode(plain, 2).keys == () and LogicalOrderByNode(plain, 2).limit is None


@pytest.mark.parametrize("sql, ordinal", [("SELECT a, b FROM t ORDER BY 0", "0"), ("SELECT a, b FROM t ORDER BY 3", "3"),
                                          ("SELECT a, b FROM t ORDER BY 1, 7 DESC LIMIT 2", "7")])
def test_ordinal_outside_the_select_list_raises_at_plan_time(sql, ordinal):
    with pytest.raises(RuntimeError, match=rf"\b{ordinal}\b"):
        buildLogicalPlan(_registry(), parseQuery(sql))


def _kotlin_compare(a, b):
    """compareValues on two boxed values."""
    ka, kb = _compare_key(a), _compare_key(b)
    return -1 if ka < kb else 1 if ka > kb else 0


def _expected(rows, keys, limit):
    """Written out independently of list.sort(reverse=...): ONE stable sort under the chained comparator, a descending key
    compares (b, a)."""
    def cmp(x, y):
        for c, desc in keys:
            r = _kotlin_compare(y[c], x[c]) if desc else _kotlin_compare(x[c], y[c])
            if r:
                return r
        return 0
    out = sorted(rows, key=functools.cmp_to_key(cmp))
    return out if limit is None else out[:limit]


NAN = float("nan")
ROWS = [[k0, k1, i] for i, (k0, k1) in enumerate(itertools.product(
    [1.5, None, NAN, -0.0, 0.0, float("-inf"), 1.5, None, -NAN],
    ["a", None, "\U0001F600", "～", "", "a"]))]
BOOL_ROWS = [[b, d, i] for i, (b, d) in enumerate(itertools.product([True, None, False, True, False], [2.0, None, NAN, -0.0, 0.0, 2.0]))]


def _ids(rows):
    return [r[-1] for r in rows]


@pytest.mark.parametrize("d0, d1", list(itertools.product((False, True), repeat=2)))
@pytest.mark.parametrize("rows", [ROWS, BOOL_ROWS], ids=["double-string", "boolean-double"])
def test_host_order_by_two_keys_in_every_direction(rows, d0, d1):
    keys = [(0, d0), (1, d1)]
    n = len(rows)
    for limit in (None, 0, 1, n, n + 5):
        op = OrderByOperator(Rows(rows), 0, keys, limit)
        got = op_map(op, lambda r: r)
        assert _ids(got) == _ids(_expected(rows, keys, limit)), (keys, limit)
        assert len(got) == (n if limit is None else min(limit, n))
        assert _ids(op_map(op, lambda r: r)) == _ids(got)            # re-opening gives the same rows


def test_host_order_by_descending_puts_null_last_and_keeps_ties_in_input_order():
    rows = [[0.0, "t0"], [None, "n0"], [NAN, "x"], [-0.0, "m"], [0.0, "t1"], [None, "n1"], [7.0, "s"], [0.0, "t2"]]
    got = op_map(OrderByOperator(Rows(rows), 0, [(0, True)]), lambda r: r[1])
    assert got == ["x", "s", "t0", "t1", "t2", "m", "n0", "n1"]       # NaN first, 0.0 before -0.0, NULL last, ties not reversed
    got = op_map(OrderByOperator(Rows(rows), 0, [(0, False)]), lambda r: r[1])
    assert got == ["n0", "n1", "m", "t0", "t1", "t2", "s", "x"]
    strs = [["a"], ["\U0001F600"], [None], ["～"], [""], ["B"]]
    assert op_map(OrderByOperator(Rows(strs), 0, [(0, True)]), lambda r: r[0]) == ["～", "\U0001F600", "a", "B", "", None]
    bools = [[False], [None], [True]]
    assert op_map(OrderByOperator(Rows(bools), 0, [(0, True)]), lambda r: r[0]) == [True, False, None]
    # the second key breaks the ties of the first, its own ties stay in input order
    rows = [[1, "b", 0], [0, "a", 1], [1, "a", 2], [1, "b", 3], [0, "a", 4]]
    assert _ids(op_map(OrderByOperator(Rows(rows), 0, [(0, True), (1, False)]), lambda r: r)) == [2, 0, 3, 1, 4]
    assert _ids(op_map(OrderByOperator(Rows(rows), 0, [(0, True), (1, False)], 3), lambda r: r)) == [2, 0, 3]


def test_order_by_operator_keeps_its_two_argument_form():
    rows = [[2.0, 0], [None, 1], [1.0, 2]]
    op = OrderByOperator(Rows(rows), 0)
    assert op.index == 0 and op.keys is None and op.limit is None
    with pytest.raises(RuntimeError, match="not opened"):
        op.next()
    assert _ids(op_map(op, lambda r: r)) == [1, 2, 0]
    op = OrderByOperator(Rows(rows), 0, [(0, True)], 2)
    with pytest.raises(RuntimeError, match="not opened"):
        op.next()
    assert _ids(op_map(op, lambda r: r)) == [0, 2]
    with pytest.raises(RuntimeError, match="not opened"):
        op.next()                                                    # closed again


def test_header_declares_and_native_binds_the_new_calls():
    text = open(os.path.join(ROOT, "include", "qe_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*int32_t\s+column;\s*int32_t\s+descending;\s*\}\s*qe_sort_key;", code)
    assert re.search(r"int32_t\s+qe_result_order_by_keys\s*\(", code) and re.search(r"int32_t\s+qe_ctx_last_sort_stats\s*\(", code)
    assert re.search(r"int32_t\s+qe_result_order_by\s*\(qe_ctx \*ctx, const qe_result \*result, int32_t column, qe_result \*\*out\);", code)
    bound = {n: (r, a) for n, r, a in N.SYMBOLS}
    assert len(bound["qe_result_order_by_keys"][1]) == 6 and len(bound["qe_ctx_last_sort_stats"][1]) == 2
    import ctypes as C
    assert C.sizeof(N.SortKey) == 8 and [f[0] for f in N.SortKey._fields_] == ["column", "descending"]
