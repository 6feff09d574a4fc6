"""The fused filter+project forms under PLACED keeps (tests/keep_pattern_reference.py): every seam of the ring's spill
rule, full chunks next to empty ones, the local form's slot exactly full, row counts chosen from the look-back's levels.

Every execution is compared bit for bit with the numpy reference (col[mask]; test_keep_patterns_cpu.py shows that it equals
the C oracle and that the patterns spill where they are meant to), and asserts the form that answered.  Consecutive
executions carry different row ids (a tag in bits 40 .. 47), so a row that an earlier execution left in a staging slot or
an LDS ring cannot pass for one of this execution's rows.  Geometries are shrunk through qe_options.tuning so that 64
chunks -- one block of the look-back -- are 64 Ki rows.
"""
import itertools
import re

import numpy as np
import pytest

from queryengine_amd import engine as E
from queryengine_amd import native as N

import keep_pattern_reference as K
from helpers import assert_columns_equal

pytestmark = pytest.mark.gpu

GEO = K.GEOMETRIES
BITS = {"ring": K.RING_BITS, "dense": K.DENSE_BITS, "two_pass": K.TWO_PASS_BITS, "local": K.LOCAL_BITS}
FORM = {"ring": N.FORM_RING, "dense": N.FORM_DENSE, "two_pass": N.FORM_TWO_PASS, "local": N.FORM_LOCAL, "per_node": N.FORM_PER_NODE}
LOCAL_SUBS = {"default": 1, "small": 4}     # sub-tiles per chunk of the local form, pinned: its chunk does not follow the remembered selectivity
_tags = itertools.count(1)


def open_ctx(form, geo, **knobs):
    if form == "per_node":
        return E.Context(device=0, exec_mode=N.EXEC_PER_NODE)
    if form == "local":
        knobs.setdefault("subs", LOCAL_SUBS[geo.name])
    return E.Context(device=0, tuning=geo.tuning(BITS[form], **knobs))


class Runner:
    """One context, one row shape, one filter literal (= one plan with its own memory): executes cases and compares."""

    def __init__(self, ctx, form, geo, shape, literal=1):
        self.ctx, self.form, self.geo, self.shape, self.literal = ctx, form, geo, shape, literal
        self.compiled = None
        self.local_chunk = None      # rows of a chunk of the local form (read_plan)
        self.overflowed = set()      # local form: the plans (by the nullability of their columns) that met a chunk which did
                                     # not fit its slot: they stay with the ring

    def read_plan(self, batch):
        """The geometry the plan REALLY has, from the #defines of its generated source: the default sub-tile is halved for
        plans whose registers or LDS tile would not fit, so the seams are placed by the plan's numbers, and the geometry table
        of keep_pattern_reference.py is checked against them."""
        if self.form == "per_node":
            self.local_chunk = 0
            return
        src = E.generated_source(self.ctx, batch, self.compiled[0], self.compiled[1])
        d = {k: int(v) for k, v in re.findall(r"#define (QE_(?:WAVES|SUB_ROWS|CHUNK_ROWS|RING|FL_RING)) (\d+)", src)}
        if self.form == "dense":
            assert d["QE_SUB_ROWS"] * d["QE_WAVES"] == self.geo.dense_tile_rows(K.ROW_BYTES[self.shape]), d
        else:
            assert d["QE_RING"] == self.geo.ring and d["QE_FL_RING"] == K.fl_ring(self.shape, self.geo), d
        if self.form in ("ring", "two_pass"):
            assert d["QE_CHUNK_ROWS"] == self.geo.chunk_rows, d
        self.local_chunk = LOCAL_SUBS.get(self.geo.name, 0) * d["QE_SUB_ROWS"]

    def want_form(self, case):
        """The form that must answer: the forced one; in the local form the ring once a chunk has kept more rows than its slot
        holds, in this execution or in an earlier one of the plan."""
        if self.form != "local":
            return FORM[self.form]
        plan = tuple(c.valid is not None for c in case.columns)
        if K.chunk_counts(case.mask, self.local_chunk).max() > K.fl_ring(self.shape, self.geo):
            self.overflowed.add(plan)
        return N.FORM_RING if plan in self.overflowed else N.FORM_LOCAL

    def run(self, pattern, n, unit=None, tag=None, mask=None):
        what = f"{self.form}/{self.geo.name}/{self.shape} {K.pattern_id(pattern)} n={n}"
        if mask is None:
            mask = K.keep_mask(pattern, n, self.geo, unit)
        case = K.build_case(self.shape, n, mask, next(_tags) % 256 if tag is None else tag, self.literal)
        want = K.expected(case.columns, mask, case.spec)
        if self.compiled is None:
            self.compiled = (self.ctx.compile(case.filter), [self.ctx.compile(p) for p in case.projections])
        batch = E.DeviceBatch.from_columns(self.ctx, case.columns)
        try:
            if self.local_chunk is None:
                self.read_plan(batch)
            res = E.filter_project(self.ctx, batch, self.compiled[0], self.compiled[1])
            form = self.ctx.last_form
            count, got = res.count, res.to_columns()
            res.free()
        finally:
            batch.free()
        want_form = self.want_form(case)
        assert form == want_form, f"{what}: form {form}, want {want_form}"
        assert count == int(mask.sum()), f"{what}: {count} rows, want {int(mask.sum())}"
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert_columns_equal(g, w, f"{what} projection {j}")
        return got


def seam_order(geo):
    """Largest k first, then small and large in turn: a sparse execution always follows one that filled the staging slots."""
    ks = sorted(K.seam_counts(geo))
    order = [ks.pop()]
    while ks:
        order.append(ks.pop(0))
        if ks:
            order.append(ks.pop())
    return order


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("geo", list(GEO.values()), ids=lambda g: g.name)
def test_ring_spill_seams(native_lib, geo, shape):
    """Chunk 1 keeps exactly k rows, at its head or in its last load groups, for every k around the spill threshold
    (ring - 129 / - 128 / - 127), each further 64, the ring size and the whole chunk; nothing else is kept, so a wrong
    prefix, a wrong staging base or a lost / doubled row at the boundary between the spilled part [0, flushed) and the
    LDS-resident part [flushed, run) of the chunk shows in the first or last row ids."""
    n = 5 * geo.chunk_rows + 129
    ctx = open_ctx("ring", geo)
    try:
        r = Runner(ctx, "ring", geo, shape)
        for k in seam_order(geo):
            for where in ("seam_head", "seam_tail"):
                r.run((where, k), n)
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("which_n", [0, 1], ids=["64C+1", "130C+7"])
@pytest.mark.parametrize("geo", list(GEO.values()), ids=lambda g: g.name)
def test_ring_full_and_empty_chunks(native_lib, geo, which_n, shape):
    """Chunks that keep everything (and spill all but the ring's tail) next to chunks that keep nothing or one row, with
    periods of 2, 3, 64 and 65 chunks against the look-back's blocks of 64: a wrong exclusive prefix moves rows by whole
    chunks.  One chunk past a block, and two blocks plus a ragged tail."""
    c = geo.chunk_rows
    n = (64 * c + 1, 130 * c + 7)[which_n]
    ctx = open_ctx("ring", geo)
    try:
        r = Runner(ctx, "ring", geo, shape)
        for p in (2, 3, 64, 65):
            r.run(("full_then_empty", p), n)
            r.run(("full_then_one", p), n)
        r.run(("all",), n)
        r.run(("none",), n)
        for length in (74, c, 3 * c + 1):
            r.run(("straddle", 2 * c - 37, length), n)
    finally:
        ctx.close()


LANE_PATTERNS = [("one_per_chunk_last",), ("first_row",), ("last_row",), ("one_per_group",), ("lane63",), ("odd_rows",), ("even_rows",)]
LANE_FORMS = [("ring", "default", {}), ("ring", "small", {}), ("ring", "default", {"stores": 5}), ("ring", "small", {"stores": 5}),
              ("dense", "default", {}), ("two_pass", "default", {}), ("local", "default", {}), ("local", "small", {}),
              ("per_node", "default", {})]


def _form_id(f):
    return f"{f[0]}-{f[1]}" + ("-vec" if f[2].get("stores") else "")


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("form", LANE_FORMS, ids=_form_id)
def test_lane_and_parity_patterns(native_lib, form, shape):
    """A lane holds rows 2l and 2l + 1 of a load group and ranks come from one ballot per parity: only odd rows, only even
    rows, only lane 63, one row per group (every lane and both parities in turn), one row per chunk, the first row, the last
    row of a ragged batch.  Sparse patterns first: in the local form they fit the chunk slots, the half-full ones (512 rows of
    a 1024-row chunk: exactly the slot of an 8-byte row) may not.  `-vec`: two rows per lane leave the ring in one store."""
    name, geo, knobs = form[0], GEO[form[1]], form[2]
    n = 5 * geo.chunk_rows + 129
    ctx = open_ctx(name, geo, **knobs)
    try:
        r = Runner(ctx, name, geo, shape)
        for pattern in LANE_PATTERNS:
            r.run(pattern, n)
    finally:
        ctx.close()


RUN_PATTERNS = [("iid", 21, 0.03), ("runs", 11, 40, 400), ("runs", 34, 5000, 50000), ("iid", 22, 0.12), ("iid", 23, 0.5), ("runs", 12, 400, 40)]
RUN_FORMS = [("ring", g, {}) for g in GEO] + [("dense", "default", {}), ("dense", "small", {}), ("two_pass", "default", {}),
                                              ("two_pass", "small", {}), ("local", "default", {}), ("local", "small", {}),
                                              ("per_node", "default", {})]


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("form", RUN_FORMS, ids=_form_id)
def test_clustered_runs_every_form(native_lib, form, shape):
    """Alternating geometric runs of kept and dropped rows (mean 40 / 400, 400 / 40, 5000 / 50000) next to i.i.d. keeps of the
    same densities, over a block of 64 chunks plus a ragged chunk: clustered keeps fill some chunks past the ring and leave
    their neighbours empty, which i.i.d. keeps never do."""
    name, geo, knobs = form[0], GEO[form[1]], form[2]
    n = 65 * geo.chunk_rows + geo.sub_rows - 1
    ctx = open_ctx(name, geo, **knobs)
    try:
        r = Runner(ctx, name, geo, shape)
        for pattern in RUN_PATTERNS:
            r.run(pattern, n)
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("geo", [GEO["default"], GEO["small"]], ids=lambda g: g.name)
def test_dense_tiles_full_next_to_empty(native_lib, geo, shape):
    """The dense form parks a tile's kept rows in LDS and resolves them one tile later: full tiles next to empty and one-row
    tiles (periods 2, 3, 64, 65 in TILES), and a ragged last tile that keeps everything."""
    tile = geo.dense_tile_rows(K.ROW_BYTES[shape])
    ctx = open_ctx("dense", geo)
    try:
        r = Runner(ctx, "dense", geo, shape)
        for n in (64 * tile + 1, 130 * tile + 7):
            for p in (2, 3, 64, 65):
                r.run(("full_then_empty", p), n, unit=tile)
                r.run(("full_then_one", p), n, unit=tile)
        r.run(("all",), 130 * tile + 7)
        r.run(("all",), 5 * tile + 129)
    finally:
        ctx.close()


def _slot_mask(n, begin, kept):
    """`kept` consecutive rows from `begin` (a multiple of 1024: one chunk of the local form whatever its sub-tile), and the
    last row of every other 1024-row block."""
    idx = np.arange(n)
    mask = idx % 1024 == 1023
    mask[begin:begin + 1024] = False
    mask[begin:begin + kept] = True
    return mask


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("geo", [GEO["default"], GEO["small"]], ids=lambda g: g.name)
def test_local_slot_exactly_full_and_one_more(native_lib, geo, shape):
    """The local form parks a chunk's kept rows in a slot of fl_ring rows (512 for rows of <= 18 bytes, else 256).  A chunk
    that keeps exactly fl_ring rows fits: the local form answers.  One row more overflows: the same execution answers through
    the ring, and so does the next one (the plan does not try the local form again).  More than 1024 chunks with one kept
    row each: the scan over the chunk counts takes more than one block."""
    slot = K.fl_ring(shape, geo)
    n = 9 * 1024 + 129
    ctx = open_ctx("local", geo)
    try:
        fits = Runner(ctx, "local", geo, shape)
        mask = _slot_mask(n, 3 * 1024, slot)
        for _ in range(2):
            fits.run(("slot_full", slot), n, mask=mask)
            assert ctx.last_form == N.FORM_LOCAL and K.chunk_counts(mask, fits.local_chunk).max() == slot
        over = Runner(ctx, "local", geo, shape, literal=2)      # another literal: a plan with its own memory
        mask = _slot_mask(n, 3 * 1024, slot + 1)
        for _ in range(2):
            over.run(("slot_full_plus_one", slot + 1), n, mask=mask)
            assert ctx.last_form == N.FORM_RING and K.chunk_counts(mask, over.local_chunk).max() == slot + 1
        fits.run(("one_per_chunk_last",), 1025 * 1024 + 5, unit=1024)
        assert ctx.last_form == N.FORM_LOCAL
    finally:
        ctx.close()


@pytest.mark.parametrize("knobs", [{}, {"lookback_k": 4, "nbuf": 3}], ids=["defaults", "k4-nbuf3"])
def test_many_chunks_behind_the_look_back(native_lib, knobs):
    """4161 chunks of 1024 rows = 65 blocks of 64 chunks and a ragged one: a look-back MAY consume a whole window of 64 block
    totals before it meets a published prefix.  Which path a wave's look-back takes (level 0 only, level 1, a consumed
    window) depends on how far the resolves trail the streaming, i.e. on timing, and cannot be forced from the data; the
    assertion is that the rows are exact whichever path was taken.  Full chunks next to one-row chunks, and long runs: a wrong
    block total moves every later row.  Also with 4 descriptor windows per look-back round and 3 LDS buffers per wave."""
    geo = GEO["small"]
    n = 64 * 64 * 1024 + 64 * 1024 + 3
    ctx = open_ctx("ring", geo, **knobs)
    try:
        r = Runner(ctx, "ring", geo, "one")
        r.run(("full_then_one", 3), n)
        r.run(("runs", 34, 5000, 50000), n)
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("form", ["ring", "dense"])
def test_same_bytes_twice_and_after_another_pattern(native_lib, form, shape):
    """Pattern A, then B (other rows, other row ids, fuller staging slots), then A again: both answers to A are byte for byte
    the same and equal to the reference -- nothing of B's execution is left in them."""
    geo = GEO["small"]
    n = 65 * geo.chunk_rows + geo.sub_rows - 1
    ctx = open_ctx(form, geo)
    try:
        r = Runner(ctx, form, geo, shape)
        first = r.run(("runs", 11, 40, 400), n, tag=7)
        r.run(("runs", 12, 400, 40), n, tag=8)
        again = r.run(("runs", 11, 40, 400), n, tag=7)
        for a, b in zip(first, again):
            assert a.data.tobytes() == b.data.tobytes()
            assert (a.valid is None) == (b.valid is None) and (a.valid is None or a.valid.tobytes() == b.valid.tobytes())
    finally:
        ctx.close()
