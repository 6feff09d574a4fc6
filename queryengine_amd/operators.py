"""Physical operators: the reference's pull protocol on top of the GPU path.

``Operator`` is ``operator/Operators.kt:5-11`` (``open / next / close``; ``next()`` returns one boxed
row or ``None``); ``forEach / map / mapTo`` are ``:13-32``.  The two GPU operators do all their work in
``open()`` -- exactly like the reference's blocking operators (``GlobalAggregationOperator.kt:10-25``)
-- and box rows lazily in ``next()``.  Operators are re-openable (``MemorySourceOperator.kt:10-12``;
the JMH harness re-runs open/next/close on one plan, ``T/SimpleSumBenchmark.java:63-94``): the input
batch is pinned to HBM once per (table, context) and reused by every ``open()``.

There is no CPU evaluation here: expressions only ever run inside libqe_hip.so.
"""
from __future__ import annotations

import contextlib
import math
import struct
from typing import Any, Callable, List, Optional, Sequence

from . import engine as E
from . import native as N
from .ast import AggregationFunction, Expression
from .table import Column, ColumnarTable


class Operator:
    def open(self) -> None:
        raise NotImplementedError

    def close(self) -> None:
        raise NotImplementedError

    def next(self) -> Optional[List[Any]]:
        raise NotImplementedError

    # Closeable.use
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def forEach(op: Operator, consumer: Callable[[List[Any]], None]) -> None:
    """operator/Operators.kt:13-23"""
    op.open()
    try:
        while True:
            row = op.next()
            if row is None:
                break
            consumer(row)
    finally:
        op.close()


def mapTo(op: Operator, result: list, mapper: Callable[[List[Any]], Any]) -> list:
    forEach(op, lambda row: result.append(mapper(row)))
    return result


def map(op: Operator, mapper: Callable[[List[Any]], Any]) -> list:   # noqa: A001 (reference name)
    return mapTo(op, [], mapper)


def _is_gpu_operator(source: Any) -> bool:
    """A source whose rows sit in HBM between its ``open()`` and ``close()``: it offers ``result()`` and ``ctx``."""
    return hasattr(source, "result") and hasattr(source, "ctx")


def _with_results(sources: Sequence[Operator], call: Callable[..., Any]) -> Any:
    """``call(*[s.result() for s in sources])`` with the sources open: opened in order, one object once however often it is
    listed, and closed in reverse order whether or not anything raises."""
    with contextlib.ExitStack() as opened:
        seen: list = []
        for s in sources:
            if not any(s is o for o in seen):
                s.open()
                opened.callback(s.close)
                seen.append(s)
        return call(*[s.result() for s in sources])


class DeviceResultOperator(Operator):
    """An operator that holds a device result.  When all its sources are GPU operators of one context its ``open()`` runs
    ``_device_call`` on their results, the rows never leave HBM, and the operator offers ``result()`` and ``ctx`` itself, so an
    operator on top works in HBM too; any other sources are drained and evaluated on the host by ``_rows_host()`` -- the
    executable statement of the subclass's semantics, and the expectation of the device tests -- and the operator has no
    ``ctx`` attribute at all.  A subclass ends its ``__init__`` with ``_set_sources``; ``_int_positions`` lists the row
    positions (negative: from the end) whose device value is a count that travels as a float."""

    _int_positions: Sequence[int] = ()

    def _set_sources(self, *sources: Operator) -> None:
        self._sources = sources
        self._on_device = all(_is_gpu_operator(s) for s in sources) and all(s.ctx is sources[0].ctx for s in sources)
        if self._on_device:
            self.ctx = sources[0].ctx
        self._result: Optional[E.Result] = None
        self._iter = None

    def _device_call(self, *results: E.Result) -> E.Result:
        raise NotImplementedError

    def _rows_host(self) -> List[List[Any]]:
        raise NotImplementedError

    def _device_rows(self):
        cols = self._result.to_columns()       # at the first next(): an operator on top that takes result() never pays it
        for i in range(len(cols[0]) if cols else 0):
            row = [c.value(i) for c in cols]
            for p in self._int_positions:
                row[p] = int(row[p])
            yield row

    def open(self) -> None:
        if self._on_device:
            self._result = _with_results(self._sources, self._device_call)
            self._iter = self._device_rows()
        else:
            self._iter = iter(self._rows_host())

    def result(self) -> E.Result:
        """The operator's columns in HBM (valid until close()); only when it ran on the device."""
        if self._result is None:
            raise RuntimeError("Operator not initialized")
        return self._result

    def next(self) -> Optional[List[Any]]:
        if self._iter is None:
            raise RuntimeError("Operator not opened")
        return next(self._iter, None)

    def close(self) -> None:
        self._iter = None
        if self._result is not None:
            self._result.free()
            self._result = None


def _compare_key(value: Any):
    """Sort key with the order of Kotlin's ``compareValues`` on the boxed types of the engine: null first, then
    ``Double.compareTo`` (total order: -0.0 < 0.0, NaN greatest), ``String.compareTo`` (UTF-16 code units),
    ``Boolean.compareTo`` (false < true), integers numerically."""
    if value is None:
        return (0,)
    if isinstance(value, bool):
        return (1, int(value))
    if isinstance(value, float):
        if value != value:
            return (1, 1, 0.0, 0)
        return (1, 0, value, 0 if (value == 0.0 and math.copysign(1.0, value) < 0) else 1)
    if isinstance(value, str):
        return (1, value.encode("utf-16-be", "surrogatepass"))
    return (1, 0, value, 1)


class OrderByOperator(Operator):
    """operator/OrderByOperator.kt:5-31: drain the source in ``open()``, stable ``sortBy`` on one column.

    A consumer of the path's output.  When the source is a GPU operator whose result sits in HBM
    (``result()``), the rows are sorted there (qe_result_order_by: key images, stable radix sort, gather) and boxed
    afterwards; any other source is drained and sorted on the host with the same ``compareValues`` order.

    ``keys`` = ``[(column0, descending), ...]`` orders by several columns (``compareBy().thenByDescending()`` on a stable
    sort: a descending key is the reversed comparator, so NULL comes last; ties keep their input order) and ``limit``
    keeps the first ``limit`` rows of that order.  On a GPU source that is qe_result_order_by_keys (top-k selection on
    the device); on the host one stable ``list.sort`` per key from the last to the first."""

    def __init__(self, source: Operator, index: int, keys: Optional[Sequence] = None, limit: Optional[int] = None):
        self.source = source
        self.index = index
        self.keys = None if keys is None else tuple((int(c), bool(d)) for c, d in keys)
        if self.keys is not None and not self.keys:
            raise ValueError("OrderByOperator: keys must not be empty")
        if limit is not None and limit < 0:
            raise ValueError("OrderByOperator: limit must not be negative")
        self.limit = limit
        self._iter = None
        self._sorted: Optional[E.Result] = None

    def open(self) -> None:
        if _is_gpu_operator(self.source):
            ctx = self.source.ctx

            def sort(res: E.Result) -> E.Result:
                if self.keys is None and self.limit is None:
                    return ctx.order_by(res, self.index)
                return ctx.order_by_keys(res, self.keys or [(self.index, False)], self.limit)

            self._sorted = _with_results([self.source], sort)
            cols = self._sorted.to_columns()
            n = self._sorted.count
            self._iter = ([c.value(i) for c in cols] for i in range(n))
            return
        data = mapTo(self.source, [], lambda row: list(row))
        # list.sort is stable, like java.util.List.sort -- also under reverse=True, which keeps ties in input order
        for column, descending in reversed(self.keys or ((self.index, False),)):
            data.sort(key=lambda row: _compare_key(row[column]), reverse=descending)
        if self.limit is not None:
            data = data[:self.limit]
        self._iter = iter(data)

    def close(self) -> None:
        self._iter = None
        if self._sorted is not None:
            self._sorted.free()
            self._sorted = None

    def next(self) -> Optional[List[Any]]:
        if self._iter is None:
            raise RuntimeError("Operator not opened")               # OrderByOperator.kt:23
        return next(self._iter, None)


def _join_key(values: Sequence[Any]):
    """The key tuple of a host join, normalised like the device's key images (DESIGN 4 `=`): every NaN is one value, -0.0
    and 0.0 are two, and a key that holds a ``None`` is no key at all (``None``: the row matches nothing)."""
    key = []
    for v in values:
        if v is None:
            return None
        if isinstance(v, float):
            key.append(("nan",) if v != v else (v, math.copysign(1.0, v)))
        else:
            key.append(v)
    return tuple(key)


class _TwoSidedJoinOperator(DeviceResultOperator):
    """What the joins of two sources share: the checks of the key and output lists and of the join type, the draining of the
    two sources (once when they are one object), the width of the NULL side of a LEFT / RIGHT / FULL join, and the loop that
    turns "the right rows this left row matches" (``_matches``, over what ``_index`` made of the right rows) into INNER / LEFT /
    SEMI / ANTI rows: left-row order, the matches of one row in the order ``_matches`` gives them, an unmatched LEFT row in its
    place with every right column ``None``.  RIGHT / FULL are the INNER / LEFT rows followed by the right rows that
    ``_matches`` never returned, in right-row order, each with ``None`` for every left column; they are told apart by their
    POSITION in the right source, so two equal right rows are two rows.  A subclass names its public attributes: ``<side>``,
    ``<side>_<key word>`` and ``<side>_out``."""

    _sides = ("left", "right")
    _key_word = "by"
    _key_counts = (0, 7)
    _join_types: Sequence[int] = (N.JOIN_INNER, N.JOIN_LEFT, N.JOIN_SEMI, N.JOIN_ANTI, N.JOIN_RIGHT, N.JOIN_FULL)
    _join_type_error = "unknown join type"

    def __init__(self, left: Operator, right: Operator, left_by: Sequence[int], right_by: Sequence[int], join_type: int,
                 left_out: Optional[Sequence[int]], right_out: Optional[Sequence[int]]):
        name, (lname, rname), (fewest, most) = type(self).__name__, self._sides, self._key_counts
        if left is None or right is None:
            raise ValueError(f"{name}: two sources")
        self._by = [int(c) for c in left_by], [int(c) for c in right_by]
        if not fewest <= len(self._by[0]) <= most or len(self._by[0]) != len(self._by[1]):
            raise ValueError(f"{name}: {fewest} to {most} {self._key_word} columns, as many on the {lname} side as on the {rname} side")
        if isinstance(join_type, bool) or join_type not in self._join_types:
            raise ValueError(f"{name}: {self._join_type_error}")
        self.join_type = int(join_type)
        self._outer = self.join_type in (N.JOIN_RIGHT, N.JOIN_FULL)                   # a tail of unmatched right rows
        self._keeps_left = self.join_type in (N.JOIN_LEFT, N.JOIN_FULL)               # an unmatched left row stays, in its place
        self._pairs = self._outer or self.join_type in (N.JOIN_INNER, N.JOIN_LEFT)
        if not self._pairs and right_out:
            raise ValueError(f"{name}: a SEMI / ANTI join has no {rname} columns")
        self._out = [None if out is None else [int(c) for c in out] for out in (left_out, right_out)]
        no_right_column = not self._pairs or (self._out[1] is not None and not self._out[1])
        if self._out[0] is not None and not self._out[0] and no_right_column:
            raise ValueError(f"{name}: no output column")
        for side, source, by, out in zip(self._sides, (left, right), self._by, self._out):
            setattr(self, side, source)
            setattr(self, f"{side}_{self._key_word}", by)
            setattr(self, f"{side}_out", out)
        self._set_sources(left, right)

    def _out_lists(self, lres: E.Result, rres: E.Result):
        """The output lists of the device call: a list that was not given is every column of its side (SEMI / ANTI: no right one)."""
        left_out, right_out = self._out
        return (list(range(lres.ncols)) if left_out is None else left_out,
                (list(range(rres.ncols)) if self._pairs else []) if right_out is None else right_out)

    def _index(self, right_rows: List[List[Any]]):
        return right_rows

    def _matches(self, row: List[Any], index) -> List[List[Any]]:
        raise NotImplementedError

    def _rows_host(self) -> List[List[Any]]:
        left, right = self._sources
        left_rows = mapTo(left, [], lambda row: list(row))
        right_rows = left_rows if right is left else mapTo(right, [], lambda row: list(row))
        left_out, right_out = self._out
        if right_out is None:
            if not self._pairs:
                right_out = []
            elif right_rows:
                right_out = list(range(len(right_rows[0])))
            elif self._keeps_left and left_rows:
                rname, jname = self._sides[1], "FULL" if self._outer else "LEFT"
                raise ValueError(f"{type(self).__name__}: {rname}_out must be given when a {jname} join's {rname} source yields no row")
            else:
                right_out = []
        if left_out is None and self._outer and right_rows and not left_rows:   # the whole right side is the tail: how many Nones?
            lname, jname = self._sides[0], "FULL" if self._keeps_left else "RIGHT"
            raise ValueError(f"{type(self).__name__}: {lname}_out must be given when a {jname} join's {lname} source yields no row")
        index = self._index(right_rows)
        out = []
        returned = set()   # RIGHT / FULL: id() of the right rows _matches has returned -- the row objects of right_rows, one per position
        for row in left_rows:
            head = [row[c] for c in (range(len(row)) if left_out is None else left_out)]
            matches = self._matches(row, index)
            if self._outer:
                returned.update(id(m) for m in matches)
            if self.join_type == N.JOIN_SEMI:
                if matches:
                    out.append(head)
            elif self.join_type == N.JOIN_ANTI:
                if not matches:
                    out.append(head)
            elif matches:
                out.extend(head + [m[c] for c in right_out] for m in matches)
            elif self._keeps_left:
                out.append(head + [None] * len(right_out))
        if self._outer:
            nleft = len(left_rows[0]) if left_out is None and left_rows else len(left_out or ())
            out.extend([None] * nleft + [r[c] for c in right_out] for r in right_rows if id(r) not in returned)
        return out


class HashJoinOperator(_TwoSidedJoinOperator):
    """Equi-join of a probe source against a build source: ``probe_keys[i]`` pairs with ``build_keys[i]`` (column
    indices).  ``join_type`` is ``native.JOIN_INNER / JOIN_LEFT / JOIN_SEMI / JOIN_ANTI / JOIN_RIGHT / JOIN_FULL``.  A row is
    the listed probe columns followed by the listed build columns (``None`` = every column of that side; SEMI and ANTI have
    no build columns); rows come in the order of a nested loop with the probe side outside: probe-row order, the matches of
    one probe row in build-row order, an unmatched LEFT row in its place with every build column ``None``.  ``JOIN_RIGHT``
    is the INNER rows and ``JOIN_FULL`` the LEFT rows, each followed by every build row that no probe row matched (a build
    row with a ``None`` key among them), once, in build-row order, every probe column ``None``; ``probe_out`` must be given
    when the probe source yields no row, as ``build_out`` must under LEFT / FULL when the build source yields none.  The
    reference has no join (Query.g4 reads one table); the operator follows ``OrderByOperator``.

    When both sources are GPU operators of one context (``result()`` and ``ctx``), the join runs on the device
    (qe_join_build + qe_join_probe) and the operator offers ``result()`` and ``ctx`` itself, so an ``OrderByOperator`` on top
    sorts in HBM too.  Any other pair of sources is drained and joined on the host with a dict from the key tuple to the
    list of build rows in order -- the executable statement of the semantics, and the expectation of the device tests."""

    _sides = ("probe", "build")
    _key_word = "keys"
    _key_counts = (1, 4)

    def __init__(self, probe: Operator, build: Operator, probe_keys: Sequence[int], build_keys: Sequence[int],
                 join_type: int = N.JOIN_INNER, probe_out: Optional[Sequence[int]] = None,
                 build_out: Optional[Sequence[int]] = None):
        super().__init__(probe, build, probe_keys, build_keys, join_type, probe_out, build_out)

    def _device_call(self, pres: E.Result, bres: E.Result) -> E.Result:
        probe_out, build_out = self._out_lists(pres, bres)
        table = self.ctx.join_build(bres, self.build_keys)
        try:
            return table.probe(pres, self.probe_keys, self.join_type, probe_out, build_out)
        finally:
            table.free()

    def _index(self, build_rows: List[List[Any]]) -> dict:
        """The key tuple -> the build rows that hold it, in build-row order."""
        table: dict = {}
        for row in build_rows:
            key = _join_key([row[c] for c in self.build_keys])
            if key is not None:
                table.setdefault(key, []).append(row)
        return table

    def _matches(self, row: List[Any], table: dict) -> List[List[Any]]:
        key = _join_key([row[c] for c in self.probe_keys])
        return table.get(key, []) if key is not None else []


def _window_min(a: float, b: float, want_max: bool) -> float:
    """MIN / MAX of two doubles as the aggregates decide them: NaN wins, -0.0 is below +0.0."""
    if a != a:
        return a
    if b != b:
        return b
    if want_max:
        return b if _compare_key(b) > _compare_key(a) else a
    return b if _compare_key(b) < _compare_key(a) else a


class WindowOperator(DeviceResultOperator):
    """Window functions over a source: every source row, sorted stably by ``partition_by`` (column indices, ascending) and
    then by ``order_by`` (``[(column, descending), ...]``, the comparator of ``OrderByOperator``), followed by one value
    per entry of ``functions`` = ``[(fn, column, offset), ...]`` or ``[(fn, column, offset, preceding, following), ...]``
    (``fn`` one of ``native.WIN_*``; ``column`` is ignored by the three ranks, ``offset`` is read by LAG / LEAD only; shorter
    tuples are padded with zeros).

    Adjacent rows share a partition when they compare equal on every partition column (``None`` is a key value, all NaNs
    are one value, -0.0 and 0.0 are two); peers are rows of a partition that compare equal on every order key.  The frame
    of an entry of three elements or fewer is ROWS BETWEEN UNBOUNDED PRECEDING AND CURRENT ROW.  A longer entry names its
    frame: ROWS BETWEEN ``preceding`` PRECEDING AND ``following`` FOLLOWING, each ``native.FRAME_UNBOUNDED`` or a row count
    in [0, 2^31), clamped to the partition -- rows ``max(start, i - preceding) .. min(end, i + following)``, which always
    hold the current row; SUM / COUNT / MIN / MAX / AVG read those rows, FIRST_VALUE / LAST_VALUE (these need a long entry)
    give the value of the first / last of them, ``None`` included; the ranks and LAG / LEAD take no frame (both must be
    0).  ROW_NUMBER, RANK (the row number of the first peer) and
    DENSE_RANK are ints; SUM / MIN / MAX / AVG skip ``None`` and are ``None`` until the partition has shown a value; COUNT
    counts the values so far (an int, like the COUNT of the aggregation operators); LAG / LEAD give the value ``offset``
    rows before / after in the partition, ``None`` beyond its edge.  The reference has no windows (Query.g4).

    When the source is a GPU operator (``result()`` and ``ctx``) the rows never leave HBM (qe_result_window, or
    qe_result_window_frames as soon as one entry names a frame) and the
    operator offers ``result()`` and ``ctx`` itself.  Any other source is drained and evaluated on the host: stable sorts
    with ``_compare_key``, then one sequential loop per partition (per row over the rows of its frame, when a frame is
    named) -- the executable statement of the semantics, and the expectation of the device tests."""

    def __init__(self, source: Operator, partition_by: Sequence[int], order_by: Sequence, functions: Sequence):
        self.source = source
        self.partition_by = [int(c) for c in partition_by]
        self.order_by = [(int(c), bool(d)) for c, d in order_by]
        # short entries stay 3-tuples (the running frame, qe_result_window); an entry that names a frame is a 5-tuple
        self.functions = [tuple(int(v) for v in ((tuple(f) + (0, 0))[:3] if len(tuple(f)) <= 3 else (tuple(f) + (0,))[:5])) for f in functions]
        self._frames = [E.window_frame_fn(f) for f in self.functions]
        if len(self.partition_by) + len(self.order_by) > 8:
            raise ValueError("WindowOperator: at most 8 partition and order columns")
        if not 1 <= len(self.functions) <= 16:
            raise ValueError("WindowOperator: 1 to 16 functions")
        for given, (fn, _, offset, preceding, following) in zip(self.functions, self._frames):
            if not N.WIN_ROW_NUMBER <= fn <= (N.WIN_LEAD if len(given) == 3 else N.WIN_LAST_VALUE):
                raise ValueError("WindowOperator: unknown window function")
            if fn in (N.WIN_LAG, N.WIN_LEAD) and not 0 <= offset < 2 ** 31:
                raise ValueError("WindowOperator: 0 <= offset < 2^31")
            if not (-1 <= preceding < 2 ** 31 and -1 <= following < 2 ** 31):
                raise ValueError("WindowOperator: preceding and following are FRAME_UNBOUNDED or in [0, 2^31)")
            if not N.WIN_SUM <= fn <= N.WIN_AVG and fn not in (N.WIN_FIRST_VALUE, N.WIN_LAST_VALUE) and (preceding, following) != (0, 0):
                raise ValueError("WindowOperator: the ranks and LAG / LEAD take no frame")
        self._int_positions = [k - len(self.functions) for k, f in enumerate(self.functions) if f[0] == N.WIN_COUNT]
        self._set_sources(source)

    def _device_call(self, res: E.Result) -> E.Result:
        return self.ctx.window(res, self.partition_by, self.order_by, self.functions)

    def _rows_host(self) -> List[List[Any]]:
        data = mapTo(self.source, [], lambda row: list(row))
        for column, descending in reversed([(c, False) for c in self.partition_by] + self.order_by):
            data.sort(key=lambda row: _compare_key(row[column]), reverse=descending)
        for fn, column, *_ in self.functions:
            if fn in (N.WIN_SUM, N.WIN_MIN, N.WIN_MAX, N.WIN_AVG):
                for row in data:
                    if isinstance(row[column], (bool, str)):
                        raise ValueError("WindowOperator: SUM / MIN / MAX / AVG need a numeric column")

        def same(a, b, columns):
            return all(_compare_key(a[c]) == _compare_key(b[c]) for c in columns)
        out = []
        begin = 0
        while begin < len(data):
            end = begin + 1
            while end < len(data) and same(data[end], data[begin], self.partition_by):
                end += 1
            part = data[begin:end]
            values = [[] for _ in self.functions]
            for k, (fn, column, offset, preceding, following) in enumerate(self._frames):
                if fn in (N.WIN_FIRST_VALUE, N.WIN_LAST_VALUE) or (N.WIN_SUM <= fn <= N.WIN_AVG and (preceding, following) != (N.FRAME_UNBOUNDED, 0)):
                    values[k] = [self._framed(part, i, fn, column, preceding, following) for i in range(len(part))]
                    continue
                rank = dense = 0
                total, count, extreme = 0.0, 0, None      # Accumulators.kt:40: a sum starts from 0.0
                for i, row in enumerate(part):
                    if i == 0 or not same(row, part[i - 1], [c for c, _ in self.order_by]):
                        rank, dense = i + 1, dense + 1
                    v = row[column] if fn >= N.WIN_SUM else None
                    if fn == N.WIN_ROW_NUMBER:
                        values[k].append(i + 1)
                    elif fn == N.WIN_RANK:
                        values[k].append(rank)
                    elif fn == N.WIN_DENSE_RANK:
                        values[k].append(dense)
                    elif fn == N.WIN_LAG:
                        values[k].append(part[i - offset][column] if i - offset >= 0 else None)
                    elif fn == N.WIN_LEAD:
                        values[k].append(part[i + offset][column] if i + offset < len(part) else None)
                    else:
                        if v is not None:
                            count += 1
                            if fn in (N.WIN_SUM, N.WIN_AVG):
                                total += float(v)
                            elif fn in (N.WIN_MIN, N.WIN_MAX):
                                extreme = float(v) if extreme is None else _window_min(extreme, float(v), fn == N.WIN_MAX)
                        if fn == N.WIN_COUNT:
                            values[k].append(count)
                        elif count == 0:
                            values[k].append(None)
                        elif fn == N.WIN_SUM:
                            values[k].append(total)
                        elif fn == N.WIN_AVG:
                            values[k].append(total / count)
                        else:
                            values[k].append(extreme)
            out.extend(row + [values[k][i] for k in range(len(self.functions))] for i, row in enumerate(part))
            begin = end
        return out

    @staticmethod
    def _framed(part, i, fn, column, preceding, following):
        """One function over the frame of row i of a partition: the rows lo .. hi, one after the other."""
        lo = 0 if preceding == N.FRAME_UNBOUNDED else max(0, i - preceding)
        hi = len(part) - 1 if following == N.FRAME_UNBOUNDED else min(len(part) - 1, i + following)
        if fn == N.WIN_FIRST_VALUE:
            return part[lo][column]
        if fn == N.WIN_LAST_VALUE:
            return part[hi][column]
        total, count, extreme = 0.0, 0, None      # Accumulators.kt:40: a sum starts from 0.0
        for row in part[lo:hi + 1]:
            v = row[column]
            if v is None:
                continue
            count += 1
            if fn in (N.WIN_SUM, N.WIN_AVG):
                total += float(v)
            elif fn in (N.WIN_MIN, N.WIN_MAX):
                extreme = float(v) if extreme is None else _window_min(extreme, float(v), fn == N.WIN_MAX)
        if fn == N.WIN_COUNT:
            return count
        if count == 0:
            return None
        return total if fn == N.WIN_SUM else total / count if fn == N.WIN_AVG else extreme


def _same_bits(a: float, b: float) -> bool:
    return struct.pack("<d", a) == struct.pack("<d", b)


class OrderedAggregateOperator(DeviceResultOperator):
    """Ordered-set aggregates per group over a source: one row per group, the groups ASCENDING by the ``group_by`` columns
    under the comparator of ``OrderByOperator`` (``None`` first; not the insertion order of the GROUP BY operators; no column =
    the whole source is one group), the group columns followed by one value per entry of ``functions`` =
    ``[(native.OSA_*, column[, fraction]), ...]``.  No function: the distinct key tuples (SELECT DISTINCT).

    Rows share a group when they compare equal on every group column (``None`` is a key value, all NaNs are one value, -0.0
    and 0.0 are two).  The values of a group for a column are its non-``None`` values ``v[0..c-1]``, ascending under the same
    comparator.  COUNT_DISTINCT counts the distinct ones (an int; 0 for none).  PERCENTILE_DISC(q) is
    ``v[max(ceil(q * float(c)) - 1, 0)]``.  PERCENTILE_CONT(q), numeric columns only, converts to float AFTER sorting and, with
    ``h = q * float(c - 1)``, ``lo = floor(h)``, ``hi = ceil(h)``, ``frac = h - lo``, is ``v[lo]`` when ``frac == 0`` or
    ``v[lo]`` and ``v[hi]`` have the same bits, else ``v[lo] + (v[hi] - v[lo]) * frac`` in exactly this order (``engine.MEDIAN``
    is q = 0.5).  MODE is the value of the longest run of equal values, the smallest of several.  The last three are ``None``
    for a group without a value.  A source without rows gives no row, or (no group column) one row of 0 and ``None``.

    When the source is a GPU operator (``result()`` and ``ctx``) the rows never leave HBM (qe_result_group_ordered) and the
    operator offers ``result()`` and ``ctx`` itself.  Any other source is drained and evaluated on the host: stable sorts with
    ``_compare_key``, then one sequential loop per group -- the executable statement of the semantics, the exact f64 formulas
    included, and the expectation of the device tests."""

    def __init__(self, source: Operator, group_by: Sequence[int], functions: Sequence):
        self.source = source
        self.group_by = [int(c) for c in group_by]
        self.functions = [E.ordered_agg(f) for f in functions]
        if len(self.group_by) > 7:
            raise ValueError("OrderedAggregateOperator: at most 7 group columns")
        if len(self.functions) > 16:
            raise ValueError("OrderedAggregateOperator: at most 16 functions")
        if not self.group_by and not self.functions:
            raise ValueError("OrderedAggregateOperator: no group column and no function")
        if any(c < 0 for c in self.group_by) or any(c < 0 for _, c, _ in self.functions):
            raise ValueError("OrderedAggregateOperator: negative column")
        for fn, _, fraction in self.functions:
            if not N.OSA_COUNT_DISTINCT <= fn <= N.OSA_MODE:
                raise ValueError("OrderedAggregateOperator: unknown function")
            if fn in (N.OSA_PERCENTILE_CONT, N.OSA_PERCENTILE_DISC) and not 0.0 <= fraction <= 1.0:
                raise ValueError("OrderedAggregateOperator: a percentile's fraction lies in [0, 1]")
        self._int_positions = [k - len(self.functions) for k, f in enumerate(self.functions) if f[0] == N.OSA_COUNT_DISTINCT]
        self._set_sources(source)

    def _device_call(self, res: E.Result) -> E.Result:
        return self.ctx.group_ordered(res, self.group_by, self.functions)

    @staticmethod
    def _evaluate(fn: int, fraction: float, v: List[Any]):
        """One function over the ascending non-None values of one group."""
        c = len(v)
        if fn == N.OSA_COUNT_DISTINCT:
            return sum(1 for i in range(c) if i == 0 or _compare_key(v[i]) != _compare_key(v[i - 1]))
        if c == 0:
            return None
        if fn == N.OSA_PERCENTILE_DISC:
            return v[max(math.ceil(fraction * float(c)) - 1, 0)]
        if fn == N.OSA_PERCENTILE_CONT:
            h = fraction * float(c - 1)
            lo, hi = math.floor(h), math.ceil(h)
            frac = h - float(lo)
            a, b = float(v[lo]), float(v[hi])
            if frac == 0.0 or _same_bits(a, b):
                return a
            diff = b - a
            step = diff * frac
            return a + step
        best, best_len, begin = None, 0, 0                  # MODE: a later run wins only when it is LONGER
        for i in range(1, c + 1):
            if i == c or _compare_key(v[i]) != _compare_key(v[begin]):
                if i - begin > best_len:
                    best, best_len = v[begin], i - begin
                begin = i
        return best

    def _rows_host(self) -> List[List[Any]]:
        data = mapTo(self.source, [], lambda row: list(row))
        for fn, column, _ in self.functions:
            if fn == N.OSA_PERCENTILE_CONT and any(isinstance(row[column], (bool, str)) for row in data):
                raise ValueError("OrderedAggregateOperator: PERCENTILE_CONT needs a numeric column")
        for column in reversed(self.group_by):
            data.sort(key=lambda row: _compare_key(row[column]))
        if not data and not self.group_by:
            return [[self._evaluate(fn, fraction, []) for fn, _, fraction in self.functions]]
        out = []
        begin = 0
        while begin < len(data):
            end = begin + 1
            while end < len(data) and all(_compare_key(data[end][c]) == _compare_key(data[begin][c]) for c in self.group_by):
                end += 1
            row = [data[begin][c] for c in self.group_by]
            for fn, column, fraction in self.functions:
                v = sorted((r[column] for r in data[begin:end] if r[column] is not None), key=_compare_key)
                row.append(self._evaluate(fn, fraction, v))
            out.append(row)
            begin = end
        return out


class SetOperator(DeviceResultOperator):
    """UNION / INTERSECT / EXCEPT of two sources of one schema (``op`` one of ``native.SET_UNION / SET_INTERSECT / SET_EXCEPT``),
    with ``all=True`` the multiset form.  Two rows are equal when they compare equal on every column the way group keys do
    (``None`` equals ``None``, all NaNs are one value, -0.0 and 0.0 are two, strings by string).  Of a tuple that occurs cL times
    on the left and cR times on the right the operator keeps: UNION 1, UNION ALL cL + cR; INTERSECT 1 if both sides hold it,
    INTERSECT ALL min(cL, cR); EXCEPT 1 if only the left holds it, EXCEPT ALL max(cL - cR, 0).

    UNION ALL yields the left rows in their order, then the right rows in theirs.  Every other form yields its rows ASCENDING by
    column 0, then column 1, .. under the comparator of ``OrderByOperator`` (``None`` first), and the k copies of a tuple are its
    first k rows in the sequence "left rows in input order, then right rows in input order": a kept row is a left row whenever
    the tuple occurs on the left.  ``left`` and ``right`` may be the same operator; it is then drained once.  The reference has
    no set operations (Query.g4 reads one table).

    When both sources are GPU operators of one context (``result()`` and ``ctx``) the rows never leave HBM (qe_result_set_op)
    and the operator offers ``result()`` and ``ctx`` itself.  Any other pair is drained and evaluated on the host: one stable
    sort per column with ``_compare_key``, then one loop over the tuples -- the executable statement of the semantics, written
    for clarity, and the expectation of the device tests."""

    def __init__(self, left: Operator, right: Operator, op: int, all: bool = False):   # noqa: A002 (the SQL word)
        if left is None or right is None:
            raise ValueError("SetOperator: two sources")
        if isinstance(op, bool) or not isinstance(op, int) or not N.SET_UNION <= op <= N.SET_EXCEPT:
            raise ValueError("SetOperator: unknown op")
        if all not in (False, True, 0, 1):
            raise ValueError("SetOperator: all is False or True")
        self.left, self.right = left, right
        self.op, self.all = int(op), bool(all)
        self._set_sources(left, right)

    def _device_call(self, lres: E.Result, rres: E.Result) -> E.Result:
        return self.ctx.set_op(lres, rres, self.op, self.all)

    @staticmethod
    def _kept(op: int, all: bool, cl: int, cr: int) -> int:   # noqa: A002
        """Copies kept of a tuple that occurs cl times on the left and cr times on the right."""
        if op == N.SET_UNION:
            return cl + cr if all else 1
        if op == N.SET_INTERSECT:
            return min(cl, cr) if all else int(cl > 0 and cr > 0)
        return max(cl - cr, 0) if all else int(cl > 0 and cr == 0)

    def _rows_host(self) -> List[List[Any]]:
        left_rows = mapTo(self.left, [], lambda row: list(row))
        right_rows = left_rows if self.right is self.left else mapTo(self.right, [], lambda row: list(row))
        widths = {len(row) for row in left_rows} | {len(row) for row in right_rows}
        if len(widths) > 1:
            raise ValueError("SetOperator: the sides differ in their column counts")
        if widths == {0}:
            raise ValueError("SetOperator: no column")
        for c in range(next(iter(widths), 0)):
            kinds = {type(row[c]) for row in left_rows + right_rows if row[c] is not None}
            if len(kinds) > 1:
                raise ValueError(f"SetOperator: column {c} differs in type between the rows")
        if self.op == N.SET_UNION and self.all:
            return left_rows + right_rows
        # (row, is left) in the sequence "left rows, then right rows"; the sorts are stable, so a tuple's left rows stay first
        data = [(row, True) for row in left_rows] + [(row, False) for row in right_rows]
        for column in reversed(range(next(iter(widths), 0))):
            data.sort(key=lambda item: _compare_key(item[0][column]))
        out = []
        begin = 0
        while begin < len(data):
            end = begin + 1
            while end < len(data) and all(_compare_key(a) == _compare_key(b) for a, b in zip(data[end][0], data[begin][0])):
                end += 1
            cl = sum(1 for _, is_left in data[begin:end] if is_left)
            k = self._kept(self.op, self.all, cl, end - begin - cl)
            out.extend(row for row, _ in data[begin:begin + k])
            begin = end
        return out


class AsofJoinOperator(_TwoSidedJoinOperator):
    """ASOF join: for every left row the ONE right row with an equal by tuple whose ``on`` value is nearest at or before it
    (``direction=native.ASOF_BACKWARD``) or at or after it (``ASOF_FORWARD``) -- for every trade the last quote of its symbol.
    ``left_by[i]`` pairs with ``right_by[i]`` (column indices, 0 to 7 of them; none: the whole input is one partition); by
    tuples are equal as hash-join keys are (every NaN one value, -0.0 and 0.0 two, strings by string) and a ``None`` in a by
    column or in ``on``, on either side, matches nothing.  ``on`` is numeric and compares like ``OrderByOperator`` compares
    (``Double.compareTo``; integers exactly).

    BACKWARD takes, of the right rows with ``on(r) <= on(l)`` (``<`` when ``strict``), the greatest ``on(r)`` and of several
    with that value the LAST right row; FORWARD, of those with ``on(r) >= on(l)`` (``>``), the smallest and of several the
    FIRST.  A row is the listed left columns followed by the listed right columns (``None`` = every column of that side), in
    left row order: every left row under ``native.JOIN_LEFT`` (the right columns ``None`` without a match), the matched ones
    under ``JOIN_INNER``.  ``left`` and ``right`` may be the same operator; it is then drained once.  The reference has no
    join (Query.g4 reads one table).

    When both sources are GPU operators of one context (``result()`` and ``ctx``) the rows never leave HBM
    (qe_result_asof_join) and the operator offers ``result()`` and ``ctx`` itself.  Any other pair is drained and joined on the
    host by a plain nested loop over ``_join_key`` and ``_compare_key`` -- the executable statement of the semantics, written
    for clarity, and the expectation of the device tests."""

    _join_types = (N.JOIN_INNER, N.JOIN_LEFT)   # a FULL ASOF join has no accepted meaning
    _join_type_error = "the join type is INNER or LEFT"

    def __init__(self, left: Operator, right: Operator, left_by: Sequence[int], right_by: Sequence[int], left_on: int, right_on: int,
                 direction: int = N.ASOF_BACKWARD, strict: bool = False, join_type: int = N.JOIN_LEFT,
                 left_out: Optional[Sequence[int]] = None, right_out: Optional[Sequence[int]] = None):
        super().__init__(left, right, left_by, right_by, join_type, left_out, right_out)
        self.left_on, self.right_on = int(left_on), int(right_on)
        if isinstance(direction, bool) or direction not in (N.ASOF_BACKWARD, N.ASOF_FORWARD):
            raise ValueError("AsofJoinOperator: unknown direction")
        if strict not in (False, True, 0, 1):
            raise ValueError("AsofJoinOperator: strict is False or True")
        self.direction, self.strict = int(direction), bool(strict)

    @staticmethod
    def _on_key(value: Any):
        if value is not None and (isinstance(value, bool) or not isinstance(value, (int, float))):
            raise ValueError("AsofJoinOperator: the on column is numeric")
        return None if value is None else _compare_key(value)

    def _match(self, row: List[Any], right_rows: List[List[Any]]) -> Optional[List[Any]]:
        """The right row that `row` matches, or None."""
        key, on = _join_key([row[c] for c in self.left_by]), self._on_key(row[self.left_on])
        if key is None or on is None:
            return None
        best, best_on = None, None
        for r in right_rows:                                   # in right row order
            r_on = self._on_key(r[self.right_on])
            if r_on is None or _join_key([r[c] for c in self.right_by]) != key:
                continue
            if isinstance(r[self.right_on], float) != isinstance(row[self.left_on], float):
                raise ValueError("AsofJoinOperator: the on column differs in type between the sides")
            if self.direction == N.ASOF_BACKWARD:
                if (r_on < on or (r_on == on and not self.strict)) and (best is None or r_on >= best_on):   # >=: the last of equals
                    best, best_on = r, r_on
            elif (r_on > on or (r_on == on and not self.strict)) and (best is None or r_on < best_on):      # <: the first of equals
                best, best_on = r, r_on
        return best

    def _matches(self, row: List[Any], right_rows: List[List[Any]]) -> List[List[Any]]:
        match = self._match(row, right_rows)
        return [] if match is None else [match]

    def _device_call(self, lres: E.Result, rres: E.Result) -> E.Result:
        left_out, right_out = self._out_lists(lres, rres)
        return self.ctx.asof_join(lres, rres, self.left_by, self.right_by, self.left_on, self.right_on, self.direction, self.strict,
                                  self.join_type, left_out, right_out)


class RangeJoinOperator(_TwoSidedJoinOperator):
    """Range join: for every left row ALL right rows with an equal by tuple whose ``on`` value lies in the left row's interval
    ``[lo, hi]`` -- all quotes in the five seconds before a trade.  ``left_by[i]`` pairs with ``right_by[i]`` (column indices, 0
    to 7 of them; none: the whole input is one partition); by tuples are equal as hash-join keys are (every NaN one value, -0.0
    and 0.0 two, strings by string) and a ``None`` in a by column, in ``lo``, ``hi`` or ``on`` matches nothing.  ``left_lo`` and
    ``left_hi`` are columns of the left (they may be the same column), ``right_on`` one of the right; all three are numeric, of
    one type, and compare like ``OrderByOperator`` compares (``Double.compareTo``; integers exactly).  ``lo_strict`` /
    ``hi_strict`` exclude that end; an empty interval matches nothing.

    A row is the listed left columns followed by the listed right columns (``None`` = every column of that side; SEMI and ANTI
    have no right columns).  Left rows come in input order, the matches of one left row ascending by ``on``, ties in right row
    order: ``native.JOIN_INNER`` the pairs, ``JOIN_LEFT`` also a row with every right column ``None`` for a left row without a
    match, ``JOIN_SEMI`` / ``JOIN_ANTI`` the left rows with / without a match, once.  ``JOIN_RIGHT`` is the INNER rows and
    ``JOIN_FULL`` the LEFT rows, each followed by every right row that no left row matched (a right row with a ``None`` by
    column or ``on`` among them), once, in right row order, every left column ``None``; ``left_out`` must be given when the
    left source yields no row.  ``left`` and ``right`` may be the same operator; it is then drained once.  The reference has
    no join (Query.g4 reads one table).

    When both sources are GPU operators of one context (``result()`` and ``ctx``) the rows never leave HBM
    (qe_result_range_join) and the operator offers ``result()`` and ``ctx`` itself.  Any other pair is drained and joined on the
    host by a plain nested loop over ``_join_key`` and ``_compare_key`` -- the executable statement of the semantics, written
    for clarity, and the expectation of the device tests."""

    def __init__(self, left: Operator, right: Operator, left_by: Sequence[int], right_by: Sequence[int], left_lo: int, left_hi: int,
                 right_on: int, lo_strict: bool = False, hi_strict: bool = False, join_type: int = N.JOIN_INNER,
                 left_out: Optional[Sequence[int]] = None, right_out: Optional[Sequence[int]] = None):
        super().__init__(left, right, left_by, right_by, join_type, left_out, right_out)
        self.left_lo, self.left_hi, self.right_on = int(left_lo), int(left_hi), int(right_on)
        if lo_strict not in (False, True, 0, 1) or hi_strict not in (False, True, 0, 1):
            raise ValueError("RangeJoinOperator: a strict flag is False or True")
        self.lo_strict, self.hi_strict = bool(lo_strict), bool(hi_strict)

    @staticmethod
    def _value_key(value: Any):
        if value is not None and (isinstance(value, bool) or not isinstance(value, (int, float))):
            raise ValueError("RangeJoinOperator: the value columns are numeric")
        return None if value is None else _compare_key(value)

    def _matches(self, row: List[Any], right_rows: List[List[Any]]) -> List[List[Any]]:
        """The right rows that `row` matches, ascending by ``on``, ties in right row order."""
        key = _join_key([row[c] for c in self.left_by])
        lo, hi = self._value_key(row[self.left_lo]), self._value_key(row[self.left_hi])
        if lo is not None and hi is not None and isinstance(row[self.left_lo], float) != isinstance(row[self.left_hi], float):
            raise ValueError("RangeJoinOperator: the value columns differ in type")
        if key is None or lo is None or hi is None:
            return []
        found = []
        for r in right_rows:                                   # in right row order
            on = self._value_key(r[self.right_on])
            if on is None or _join_key([r[c] for c in self.right_by]) != key:
                continue
            if isinstance(r[self.right_on], float) != isinstance(row[self.left_lo], float):
                raise ValueError("RangeJoinOperator: the value columns differ in type")
            if (on > lo or (on == lo and not self.lo_strict)) and (on < hi or (on == hi and not self.hi_strict)):
                found.append((on, r))
        found.sort(key=lambda item: item[0])                   # stable: ties stay in right row order
        return [r for _, r in found]

    def _device_call(self, lres: E.Result, rres: E.Result) -> E.Result:
        left_out, right_out = self._out_lists(lres, rres)
        return self.ctx.range_join(lres, rres, self.left_by, self.right_by, self.left_lo, self.left_hi, self.right_on, self.lo_strict,
                                   self.hi_strict, self.join_type, left_out, right_out)


class ColumnarScanOperator(Operator):
    """Scan leaf over a ColumnarTable (replaces MemorySourceOperator.kt:5-36).

    As a row source it reuses ONE row buffer and nulls it on close, like the reference
    (``:8,15,26-32``).  The GPU operators do not pull rows from it: they take ``columns()``."""

    def __init__(self, table: ColumnarTable, projection: Sequence[str]):
        self.table = table
        self.projection = list(projection)
        self._columns = [table.column(name) for name in self.projection]   # raises "Unknown field" like MemoryTable.kt:11
        self._idx = 0
        self._row: List[Any] = [None] * len(self._columns)

    def columns(self) -> List[Column]:
        return self._columns

    def open(self) -> None:
        self._idx = 0

    def close(self) -> None:
        for j in range(len(self._row)):
            self._row[j] = None

    def next(self) -> Optional[List[Any]]:
        i = self._idx
        if i >= self.table.nrows:
            return None
        self._idx = i + 1
        for j, c in enumerate(self._columns):
            self._row[j] = c.value(i)
        return self._row

    def device_batch(self, ctx: E.Context) -> E.DeviceBatch:
        """Pin the projected columns to HBM once per context; later opens reuse the batch."""
        cache = self.table.__dict__.setdefault("_device_batches", {})
        # batches of contexts that were closed meanwhile are dropped (their handles died with the context)
        for k in [k for k, v in cache.items() if v.ctx.handle is None or v.handle is None]:
            del cache[k]
        key = (id(ctx), tuple(self.projection))
        b = cache.get(key)
        # id() values are recycled after a Context is collected: a hit only counts if the batch belongs to THIS context
        if b is None or b.ctx is not ctx or b.handle is None or ctx.handle is None:
            b = E.DeviceBatch.from_columns(ctx, self._columns)
            cache[key] = b
        return b


class GpuFilterProjectOperator(Operator):
    """Projection(Filter(Scan)) fused into one GPU operator.

    Replaces FilterOperator (operator/FilterOperator.kt:5-26) + ProjectionOperator
    (operator/ProjectionOperator.kt:5-21) / the generated CompiledProjectionOperator
    (evaluator/BytecodeCompiler.kt:37-132).  ``filter`` may be None."""

    def __init__(self, ctx: E.Context, source: ColumnarScanOperator, filter: Optional[Expression],
                 projections: Sequence[Expression]):
        self.ctx = ctx
        self.source = source
        # compileExpression at plan time (Planner.kt:35,44)
        self._filter = ctx.compile(filter) if filter is not None else None
        self._projections = [ctx.compile(p) for p in projections]
        self._result: Optional[E.Result] = None
        self._columns: Optional[List[Column]] = None
        self._idx = 0
        self._count = 0

    def open(self) -> None:
        self.source.open()
        batch = self.source.device_batch(self.ctx)
        self._result = E.filter_project(self.ctx, batch, self._filter, self._projections)
        self._count = self._result.count
        self._columns = None
        self._idx = 0

    def result(self) -> E.Result:
        """The columnar result in HBM (valid until close())."""
        if self._result is None:
            raise RuntimeError("Operator not initialized")   # CsvSourceOperator.kt:49
        return self._result

    def next(self) -> Optional[List[Any]]:
        if self._result is None:
            raise RuntimeError("Operator not initialized")
        if self._columns is None:
            self._columns = self._result.to_columns()       # one D2H per column, then rows are boxed lazily
        i = self._idx
        if i >= self._count:
            return None
        self._idx = i + 1
        return [c.value(i) for c in self._columns]          # a fresh row per call (ProjectionOperator.kt:18)

    def close(self) -> None:
        if self._result is not None:
            self._result.free()
        self._result = None
        self._columns = None
        self.source.close()


class GpuGlobalAggregationOperator(Operator):
    """GlobalAggregation(Projection(Filter(Scan))) as one fused GPU reduction.

    Replaces GlobalAggregationOperator (operator/GlobalAggregationOperator.kt:7-36) over the inner
    projection: one result row, nulls skipped, empty input => null (COUNT => count)."""

    def __init__(self, ctx: E.Context, source: ColumnarScanOperator, filter: Optional[Expression],
                 expressions: Sequence[Expression], aggregateFunctions: Sequence[AggregationFunction]):
        self.ctx = ctx
        self.source = source
        self._filter = ctx.compile(filter) if filter is not None else None
        self._exprs = [ctx.compile(e) for e in expressions]
        self._aggs = [int(a) for a in aggregateFunctions]
        self._row: Optional[List[Any]] = None

    def open(self) -> None:
        self.source.open()
        batch = self.source.device_batch(self.ctx)
        vals, _ = E.filter_aggregate(self.ctx, batch, self._filter, self._exprs, self._aggs)
        # CountAccumulator.finish returns an Int (Accumulators.kt:26-36)
        self._row = [int(v) if a == int(AggregationFunction.COUNT) else v for v, a in zip(vals, self._aggs)]

    def next(self) -> Optional[List[Any]]:
        res, self._row = self._row, None      # GlobalAggregationOperator.kt:32-36
        return res

    def close(self) -> None:
        self._row = None
        self.source.close()


class GpuGroupByAggregationOperator(Operator):
    """GroupByAggregation(Projection(Filter(Scan))) on the GPU.

    Replaces GroupByAggregationOperator (operator/GroupByAggregationOperator.kt:7-76) over the inner projection:
    one row [keys..., finished accumulators...] per group, in insertion order of the groups; null is a key value."""

    def __init__(self, ctx: E.Context, source: ColumnarScanOperator, filter: Optional[Expression],
                 keyExpressions: Sequence[Expression], expressions: Sequence[Expression],
                 aggregateFunctions: Sequence[AggregationFunction]):
        self.ctx = ctx
        self.source = source
        self._filter = ctx.compile(filter) if filter is not None else None
        self._keys = [ctx.compile(e) for e in keyExpressions]
        self._exprs = [ctx.compile(e) for e in expressions]
        self._aggs = [int(a) for a in aggregateFunctions]
        self._rows: Optional[List[List[Any]]] = None
        self._idx = 0

    def open(self) -> None:
        self.source.open()
        batch = self.source.device_batch(self.ctx)
        res = E.filter_groupby(self.ctx, batch, self._filter, self._keys, self._exprs, self._aggs)
        cols = res.to_columns()
        res.free()
        nk = len(self._keys)
        rows = []
        for i in range(len(cols[0]) if cols else 0):
            row = [c.value(i) for c in cols]
            for a, fn in enumerate(self._aggs):          # CountAccumulator.finish returns an Int (Accumulators.kt:26-36)
                if fn == int(AggregationFunction.COUNT) and row[nk + a] is not None:
                    row[nk + a] = int(row[nk + a])
            rows.append(row)
        self._rows = rows
        self._idx = 0

    def next(self) -> Optional[List[Any]]:
        if self._rows is None:
            raise RuntimeError("Operator not opened")      # GroupByAggregationOperator.kt:57
        if self._idx >= len(self._rows):
            return None
        self._idx += 1
        return self._rows[self._idx - 1]

    def close(self) -> None:
        self._rows = None
        self.source.close()


class GpuFinishProjectionOperator(Operator):
    """The projection the reference puts on top of an aggregation (``groupByFinish``, RewriteAggregates.kt:29-47):
    re-orders / combines the few aggregated rows.  The rows of the blocking source are pinned as one small batch and
    the expressions run on the GPU like any other projection (no CPU evaluation)."""

    def __init__(self, ctx: E.Context, source: Operator, sourceTypes: Sequence, expressions: Sequence[Expression]):
        self.ctx = ctx
        self.source = source
        self.sourceTypes = list(sourceTypes)
        self.expressions = list(expressions)
        self._compiled = [ctx.compile(e) for e in expressions]
        self._rows: Optional[List[List[Any]]] = None
        self._idx = 0

    def open(self) -> None:
        from .ast import ColumnExpression
        rows = map(self.source, lambda r: list(r))
        if not rows:
            self._rows = []
            self._idx = 0
            return
        cols = []
        for j, t in enumerate(self.sourceTypes):
            vals = [r[j] for r in rows]
            if t.name == "DOUBLE":
                vals = [float(v) if v is not None else None for v in vals]   # COUNT arrives as an Int
            cols.append(Column.from_values(t, vals))
        batch = E.DeviceBatch.from_columns(self.ctx, cols)
        res = E.filter_project(self.ctx, batch, None, self._compiled)
        out = res.to_columns()
        res.free()
        batch.free()
        result = []
        for i in range(len(rows)):
            row = [c.value(i) for c in out]
            for k, e in enumerate(self.expressions):   # a bare reference to a COUNT column keeps the Int
                if isinstance(e, ColumnExpression) and isinstance(rows[i][e.index], int) and not isinstance(rows[i][e.index], bool):
                    row[k] = rows[i][e.index]
            result.append(row)
        self._rows = result
        self._idx = 0

    def next(self) -> Optional[List[Any]]:
        if self._rows is None:
            raise RuntimeError("Operator not initialized")
        if self._idx >= len(self._rows):
            return None
        self._idx += 1
        return self._rows[self._idx - 1]

    def close(self) -> None:
        self._rows = None
