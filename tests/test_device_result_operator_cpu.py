"""The protocol that the six operators holding a device result share (``DeviceResultOperator``), without a GPU: stub sources
that record their calls, and a stub context whose device call returns a stub result or raises."""
import pytest

from queryengine_amd import native as N
from queryengine_amd.operators import (AsofJoinOperator, DeviceResultOperator, HashJoinOperator, OrderByOperator,
                                       OrderedAggregateOperator, RangeJoinOperator, SetOperator, WindowOperator)


class StubColumn:
    def __init__(self, values):
        self.values = values

    def __len__(self):
        return len(self.values)

    def value(self, i):
        return self.values[i]


class StubResult:
    ncols = 2
    count = 2

    def __init__(self, log, name):
        self.log, self.name, self.boxed = log, name, 0

    def to_columns(self):
        self.boxed += 1
        return [StubColumn([1.0, 2.0]), StubColumn([3.0, 4.0])]

    def free(self):
        self.log.append(("free", self.name))


class StubContext:
    """Every device call of the six operators: logs itself, then returns a result or raises."""

    def __init__(self, log, fail=False):
        self.log, self.fail = log, fail

    def _call(self, name, *results):
        self.log.append((name,) + tuple(r.name for r in results))
        if self.fail:
            raise RuntimeError("device call failed")
        return StubResult(self.log, "out")

    def window(self, res, *args):
        return self._call("call", res)

    def group_ordered(self, res, *args):
        return self._call("call", res)

    def set_op(self, lres, rres, *args):
        return self._call("call", lres, rres)

    def asof_join(self, lres, rres, *args):
        return self._call("call", lres, rres)

    def range_join(self, lres, rres, *args):
        return self._call("call", lres, rres)

    def join_build(self, bres, keys):      # the join: the table is built from the build side and probed with the probe side
        ctx = self

        class Table:
            def probe(self, pres, *args):
                return ctx._call("call", pres, bres)

            def free(self):
                ctx.log.append(("table free",))

        return Table()


class GpuSource:
    """A source that looks like a GPU operator: open / close / result / ctx."""

    def __init__(self, ctx, name):
        self.ctx, self.name, self.is_open = ctx, name, False

    def open(self):
        self.ctx.log.append(("open", self.name))
        self.is_open = True

    def close(self):
        self.ctx.log.append(("close", self.name))
        self.is_open = False

    def result(self):
        assert self.is_open
        return StubResult(self.ctx.log, self.name)


class HostSource:
    """A source without result() and ctx."""

    def open(self):
        self.rows = iter([[1.0, 2.0], [1.0, 3.0]])

    def close(self):
        self.rows = None

    def next(self):
        return next(self.rows, None)


# name -> (sources it takes, constructor over those sources)
OPERATORS = {
    "join": (2, lambda a, b: HashJoinOperator(a, b, [0], [0])),
    "window": (1, lambda a: WindowOperator(a, [0], [(1, False)], [(N.WIN_ROW_NUMBER, 0, 0)])),
    "ordered": (1, lambda a: OrderedAggregateOperator(a, [0], [(N.OSA_MODE, 1)])),
    "setop": (2, lambda a, b: SetOperator(a, b, N.SET_UNION)),
    "asof": (2, lambda a, b: AsofJoinOperator(a, b, [], [], 1, 1)),
    "range": (2, lambda a, b: RangeJoinOperator(a, b, [], [], 0, 1, 1)),
}
ALL = sorted(OPERATORS)
TWO_SIDED = [name for name in ALL if OPERATORS[name][0] == 2]


def make(name, fail=False, same=False):
    log = []
    ctx = StubContext(log, fail)
    nsources, build = OPERATORS[name]
    sources = [GpuSource(ctx, "a")] * 2 if same else [GpuSource(ctx, "ab"[i]) for i in range(nsources)]
    return build(*sources[:nsources]), log, ctx


@pytest.mark.parametrize("name", ALL)
def test_is_a_device_result_operator(name):
    op, _, ctx = make(name)
    assert isinstance(op, DeviceResultOperator) and op.ctx is ctx


@pytest.mark.parametrize("name", ALL)
def test_before_open(name):
    op, log, _ = make(name)
    with pytest.raises(RuntimeError, match="^Operator not opened$"):
        op.next()
    with pytest.raises(RuntimeError, match="^Operator not initialized$"):
        op.result()
    assert log == []


@pytest.mark.parametrize("name", ALL)
def test_sources_open_in_order_and_close_in_reverse(name):
    op, log, _ = make(name)
    op.open()
    names = ["a", "b"][:OPERATORS[name][0]]
    calls = [e for e in log if e[0] != "table free"]
    assert calls == [("open", s) for s in names] + [("call",) + tuple(names)] + [("close", s) for s in reversed(names)]
    if name == "join":
        assert log.index(("table free",)) < log.index(("close", "b"))      # the table goes before its build side does
    assert op.result().name == "out"
    op.close()


@pytest.mark.parametrize("name", ALL)
def test_sources_closed_when_the_device_call_raises(name):
    op, log, _ = make(name, fail=True)
    with pytest.raises(RuntimeError, match="device call failed"):
        op.open()
    names = ["a", "b"][:OPERATORS[name][0]]
    assert [e for e in log if e[0] == "close"] == [("close", s) for s in reversed(names)]
    assert op._result is None
    with pytest.raises(RuntimeError, match="^Operator not initialized$"):
        op.result()
    op.close()
    assert not any(e[0] == "free" for e in log)


@pytest.mark.parametrize("name", TWO_SIDED)
def test_one_object_as_both_sources_is_opened_once(name):
    op, log, _ = make(name, same=True)
    op.open()
    assert [e for e in log if e[0] != "table free"] == [("open", "a"), ("call", "a", "a"), ("close", "a")]
    op.close()


@pytest.mark.parametrize("name", ALL)
def test_rows_are_boxed_at_the_first_next(name):
    op, _, _ = make(name)
    op.open()
    res = op.result()
    assert res.boxed == 0
    assert op.next() == [1.0, 3.0] and res.boxed == 1
    assert op.next() == [2.0, 4.0] and op.next() is None and res.boxed == 1
    op.close()


@pytest.mark.parametrize("name", ALL)
def test_close_frees_once_and_result_raises_again(name):
    op, log, _ = make(name)
    op.open()
    op.close()
    op.close()
    assert log.count(("free", "out")) == 1
    with pytest.raises(RuntimeError, match="^Operator not initialized$"):
        op.result()
    with pytest.raises(RuntimeError, match="^Operator not opened$"):
        op.next()
    op.open()                                                              # re-openable
    assert op.result().name == "out"
    op.close()
    assert log.count(("free", "out")) == 2


@pytest.mark.parametrize("name", ALL)
def test_no_ctx_with_a_source_that_is_no_gpu_operator(name):
    nsources, build = OPERATORS[name]
    ctx = StubContext([])
    for sources in ([HostSource(), HostSource()], [GpuSource(ctx, "a"), HostSource()], [HostSource(), GpuSource(ctx, "b")]):
        if nsources == 1 and not isinstance(sources[0], HostSource):
            continue
        assert not hasattr(build(*sources[:nsources]), "ctx")


@pytest.mark.parametrize("name", TWO_SIDED)
def test_no_ctx_with_sources_of_two_contexts(name):
    op = OPERATORS[name][1](GpuSource(StubContext([]), "a"), GpuSource(StubContext([]), "b"))
    assert not hasattr(op, "ctx")


def test_counts_are_ints():
    op = WindowOperator(GpuSource(StubContext([]), "a"), [], [], [(N.WIN_COUNT, 0, 0)])
    op.open()
    row = op.next()
    assert row == [1.0, 3] and isinstance(row[1], int) and isinstance(row[0], float)
    op.close()
    op = OrderedAggregateOperator(GpuSource(StubContext([]), "a"), [0], [(N.OSA_COUNT_DISTINCT, 1)])
    op.open()
    row = op.next()
    assert row == [1.0, 3] and isinstance(row[1], int)
    op.close()


def test_order_by_stays_without_result_and_ctx():
    log = []
    ctx = StubContext(log)
    ctx.order_by = lambda res, index: ctx._call("call", res)
    op = OrderByOperator(GpuSource(ctx, "a"), 0)
    op.open()
    assert log == [("open", "a"), ("call", "a"), ("close", "a")]
    assert not hasattr(op, "result") and not hasattr(op, "ctx")
    assert op.next() == [1.0, 3.0]
    op.close()
    assert log.count(("free", "out")) == 1
