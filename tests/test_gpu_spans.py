"""Spanning depth on the device (hicmi_span_begin / _add_pairs / _finish / _file) against
tests/span_reference.py, for HICMI_SPANS_PLAIN unset, =1 and =0.  Marks, depths, counters and picks are integers and the
ratio behind a pick is one IEEE division on both sides, so every comparison is exact: there are no tolerances."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import buildmap_reference as bref
import liftmap_reference as lref
import span_reference as ref

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -5
# Both mark forms give the same bits by design: these tests hold each to the reference but cannot tell which kernel ran; that
# the switch is read per call is checked from the source in tests/test_spans_cpu.py.
FORMS = {"default": {}, "plain": {"HICMI_SPANS_PLAIN": "1"}, "combine": {"HICMI_SPANS_PLAIN": "0"}}
FORM_NAMES = ["default", "plain", "combine"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    with open(os.path.join(ROOT, "hic_genome_assembler_amd", "csrc", "hicmi_internal.h")) as fh:
        text = fh.read()
    value = re.search(r"static constexpr int %s = ([^;]+);" % name, text).group(1)
    return 1 << _constant(value.split("<<")[1].strip()) if "<<" in value else int(value)


SLICE, SLOTS, TILE, WIDTH = (_constant(k) for k in ("SPAN_SLICE", "SPAN_SLOTS", "SPAN_SCAN_TILE", "SPAN_SCAN_WIDTH"))
COUNTS = [1, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 5000]
STEP, FLANK = 500, 3
# three chromosomes of mixed orientations on the 40 odd scaffolds (sizes 1, 999, 1000, 1001, 3007 and three of 70,000)
CHROMS = [[(3, "+"), (0, "-"), (4, "-"), (17, "+"), (1, "-"), (2, "+"), (7, "-")],
          [(38, "-"), (5, "-"), (6, "+"), (9, "-"), (8, "+"), (11, "+"), (12, "-"), (13, "-")],
          [(20, "-"), (21, "+"), (22, "-"), (24, "+"), (23, "-")]]


def _set_form(monkeypatch, form):
    for key in ("HICMI_SPANS_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS", "HICMI_BUILDMAP_PLAIN", "HICMI_LIFTMAP_PLAIN"):
        monkeypatch.delenv(key, raising=False)
    for key, value in FORMS[form].items():
        monkeypatch.setenv(key, value)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _scaffolds():
    names, sizes = bref.odd_scaffolds()
    sizes.setflags(write=False)
    return names, sizes


@functools.lru_cache(maxsize=None)
def _tables(gap, drop):
    _names, sizes = _scaffolds()
    return _frozen(*lref.layout(CHROMS, sizes, gap, drop_unplaced=drop))


@functools.lru_cache(maxsize=None)
def _pool():
    """5,000 pairs: most of them inside one chromosome, some in one cell, some between chromosomes, some anywhere."""
    _names, sizes = _scaffolds()
    rng = np.random.default_rng(5)
    n = COUNTS[-1]
    members = [np.array([s for s, _o in ch]) for ch in CHROMS]
    ch = rng.integers(0, 3, n)
    sa = np.array([rng.choice(members[c], p=sizes[members[c]] / sizes[members[c]].sum()) for c in ch])
    sb = np.array([rng.choice(members[c], p=sizes[members[c]] / sizes[members[c]].sum()) for c in ch])
    pa = 1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64)
    kind = rng.integers(0, 10, n)
    near = kind <= 2                                          # a short distance on one scaffold: many in one cell
    sb[near] = sa[near]
    pb[near] = np.clip(pa[near] + rng.integers(-700, 700, near.sum()), 1, sizes[sa[near]])
    anywhere = kind == 9
    sb[anywhere] = rng.integers(0, 40, anywhere.sum())
    pb[anywhere] = 1 + np.floor(rng.random(anywhere.sum()) * sizes[sb[anywhere]]).astype(np.int64)
    return _frozen(sa.astype(np.int32), pa, sb.astype(np.int32), pb)


def _first(pairs, n):
    return tuple(a[:n] for a in pairs)


def _records(sizes, tables, step):
    """The records of a report, and every sequence as one record."""
    scaf, junc = ref.report_records(sizes, tables, step)
    _cell_first, seq_first, _n = ref.number_cells(sizes, tables, step)
    whole = [(int(a), int(b) - 1, int(a), int(b)) for a, b in zip(seq_first[:-1], seq_first[1:]) if b > a]
    return np.asarray(list(scaf.values()) + list(junc.values()) + whole, np.int64).reshape(-1, 4)


def _want(pairs, sizes, tables, step, max_span, flank, recs):
    D, counters, _marks = ref.depth(pairs, sizes, tables, step, max_span)
    cell_first, seq_first, n = ref.number_cells(sizes, tables, step)
    terminators = seq_first[1:][seq_first[1:] > seq_first[:-1]] - 1
    assert len(D) == n and not D[terminators].any()
    return cell_first, ref.picks(D, flank, recs), counters, D, terminators


def _run(sizes, tables, step, max_span, parts, flank, recs):
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        cell_first = ctx.span_begin(sizes, *tables, step, max_span)
        for p in parts:
            ctx.span_add_pairs(*p)
        return (cell_first,) + ctx.span_finish(flank, recs)


def _same(got, want):
    cell_first, picks, counters, D, terminators = want
    assert got[0].dtype == np.int64 and got[0].tolist() == cell_first.tolist()
    assert got[3].dtype == np.uint64 and got[3].shape == D.shape and got[3].tobytes() == D.tobytes()
    assert not got[3][terminators].any()                                    # the depth at every terminator is 0
    assert got[2].dtype == np.uint64 and got[2].tolist() == counters.tolist()
    assert got[1].dtype == np.int64 and got[1].shape == picks.shape and got[1].tolist() == picks.tolist()


# ---- pair counts, split calls, kinds of pairs ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_pool(n, gap, drop, max_span):
    _names, sizes = _scaffolds()
    tables = _tables(gap, drop)
    recs = _records(sizes, tables, STEP)
    return recs, _want(_first(_pool(), n), sizes, tables, STEP, max_span, FLANK, recs)


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("n", COUNTS)
def test_pair_counts_at_the_wave_workgroup_and_slice_edges(n, form, monkeypatch):
    _names, sizes = _scaffolds()
    recs, want = _want_pool(n, 100, False, 0)
    _set_form(monkeypatch, form)
    _same(_run(sizes, _tables(100, False), STEP, 0, [_first(_pool(), n)], FLANK, recs), want)


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", [0, 1, 100])
def test_every_kind_of_pair_and_the_five_counters(gap, drop, form, monkeypatch):
    _names, sizes = _scaffolds()
    for max_span in (0, 20000):
        recs, want = _want_pool(COUNTS[-1], gap, drop, max_span)
        marked, one_cell, far, trans, unlifted = want[2].tolist()
        assert marked > 1500 and one_cell > 300 and trans > 100 and (unlifted > 100) == drop and (far > 300) == (max_span > 0)
        assert marked + one_cell + far + trans + unlifted == COUNTS[-1]
        assert (want[1][:, 0] >= 0).sum() > 10 and (want[1][:, 0] < 0).sum() >= 10      # picks that compete and records where nothing does
        _set_form(monkeypatch, form)
        _same(_run(sizes, _tables(gap, drop), STEP, max_span, [_pool()], FLANK, recs), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_three_calls_equal_one(form, monkeypatch):
    _names, sizes = _scaffolds()
    recs, want = _want_pool(COUNTS[-1], 100, True, 0)
    pairs = _pool()
    cuts = [0, 100, 2500, COUNTS[-1]]
    parts = [tuple(a[cuts[k]:cuts[k + 1]] for a in pairs) for k in range(3)] + [tuple(a[:0] for a in pairs)]
    _set_form(monkeypatch, form)
    _same(_run(sizes, _tables(100, True), STEP, 0, parts, FLANK, recs), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_hot_slots_are_exact(form, monkeypatch):
    """100,000 copies of one pair: two hot slots."""
    _names, sizes = _scaffolds()
    tables = _tables(100, False)
    pairs = tuple(np.full(100000, v, dtype=t) for v, t in ((3, np.int32), (1234, np.int64), (17, np.int32), (69000, np.int64)))
    recs = _records(sizes, tables, STEP)
    want = _want(pairs, sizes, tables, STEP, 0, FLANK, recs)
    assert want[2].tolist() == [100000, 0, 0, 0, 0] and set(want[3].tolist()) == {0, 100000}
    _set_form(monkeypatch, form)
    _same(_run(sizes, tables, STEP, 0, [pairs], FLANK, recs), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_a_slice_with_more_slots_than_the_table_holds(form, monkeypatch):
    """Pair k marks the cells 2 k and 2 k + 1: a slice of the combining form meets 2 x SLICE distinct slots, more than its
    table has, so marks fall back to direct atomic adds; then 1,000 pairs more."""
    n_cells = 2 * (SLICE + 1000)
    assert 2 * SLICE > SLOTS
    sizes = np.array([n_cells], np.int64)
    tables = lref.identity(sizes)
    k = np.arange(SLICE + 1000, dtype=np.int64)
    pairs = (np.zeros(len(k), np.int32), 2 * k + 1, np.zeros(len(k), np.int32), 2 * k + 2)
    recs = [(0, n_cells - 1, 0, n_cells), (5, 700, 0, n_cells)]
    want = _want(pairs, sizes, tables, 1, 0, 2, recs)
    assert want[3].tolist() == [1, 0] * (SLICE + 1000) and want[2][0] == SLICE + 1000
    _set_form(monkeypatch, form)
    _same(_run(sizes, tables, 1, 0, [pairs], 2, recs), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_max_span_at_the_limit_and_one_beyond(form, monkeypatch):
    sizes = np.array([3000, 2000], np.int64)
    tables = lref.layout([[(0, "+"), (1, "-")]], sizes, 100)
    # base 2,500 of the first scaffold and base 1,600 of the reversed second one (lifted: 3,100 + 401) are 1,001 apart
    pairs = (np.array([0, 0, 0], np.int32), np.array([2500, 2500, 100], np.int64), np.array([1, 0, 0], np.int32), np.array([1600, 1499, 1101], np.int64))
    qa, xa, qb, xb = ref.lift(pairs, sizes, tables)
    assert np.abs(xa - xb).tolist() == [1001, 1001, 1001]
    recs = [(0, 49, 0, 50)]
    _set_form(monkeypatch, form)
    for max_span, counters in ((1001, [3, 0, 0, 0, 0]), (1000, [0, 0, 3, 0, 0]), (0, [3, 0, 0, 0, 0]), (1, [0, 0, 3, 0, 0])):
        want = _want(pairs, sizes, tables, 100, max_span, 2, recs)
        assert want[2].tolist() == counters
        _same(_run(sizes, tables, 100, max_span, [pairs], 2, recs), want)


# ---- cell totals: the edges of the scan ------------------------------------------------------------------------------------------------
CELL_TOTALS = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 5 * TILE + 5, WIDTH * TILE + 1]


@functools.lru_cache(maxsize=None)
def _scan_case(n_cells):
    """Two sequences of one scaffold each (one when there is one cell), a cell per base, and 3,000 pairs inside them."""
    sizes = np.array([n_cells - n_cells // 2] + ([n_cells // 2] if n_cells > 1 else []), np.int64)
    tables = lref.identity(sizes)
    rng = np.random.default_rng(n_cells)
    n = 3000
    s = rng.integers(0, len(sizes), n)
    pa = 1 + np.floor(rng.random(n) * sizes[s]).astype(np.int64)
    pb = np.clip(pa + np.floor(np.exp(rng.uniform(0, np.log(4.0 * n_cells), n))).astype(np.int64) * rng.choice([-1, 1], n), 1, sizes[s])
    pairs = (s.astype(np.int32), pa, s.astype(np.int32), pb)
    first = int(sizes[0])
    recs = [(0, min(first - 1, 128), 0, first)] + ([(first, min(n_cells - 1, first + 64), first, n_cells)] if n_cells > 1 else [])
    if first > 2 * TILE + 1:                                                  # records across the ends of tiles
        recs += [(TILE - 30, TILE + 98, 0, first), (2 * TILE - 1, 2 * TILE, 0, first)]
    want = _want(pairs, sizes, tables, 1, 0, 4, recs)
    _frozen(want[3])
    return sizes, tables, pairs, recs, want


@pytest.mark.parametrize("form", ["default", "plain"])
@pytest.mark.parametrize("n_cells", CELL_TOTALS)
def test_cell_totals_at_the_tile_edges_and_past_the_second_level(n_cells, form, monkeypatch):
    sizes, tables, pairs, recs, want = _scan_case(n_cells)
    assert len(want[3]) == n_cells and (n_cells < 63 or want[3].max() > 5)
    _set_form(monkeypatch, form)
    _same(_run(sizes, tables, 1, 0, [pairs], 4, recs), want)


def test_more_than_2_to_the_27_cells_are_refused():
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        with pytest.raises(_lib.HicmiError) as exc:
            ctx.span_begin([2 ** 27, 1], [0, 1], [0, 0], [0, 0], [2 ** 27, 1], 1)
        assert "error %d:" % EUNSUPPORTED in str(exc.value)
        with pytest.raises(_lib.HicmiError):
            ctx.span_finish(1, [])                                            # nothing was opened


# ---- 64-bit positions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
def test_scaffolds_of_2_to_the_33_at_a_step_of_2_to_the_20(form, monkeypatch):
    L, step = 2 ** 33, 2 ** 20
    sizes = np.array([L, L, L], dtype=np.int64)
    tables = lref.layout([[(0, "+"), (1, "-"), (2, "+")]], sizes, 100)
    edge = np.array([1, 2, step, step + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, L - step, L - step + 1, L - 1, L], dtype=np.int64)
    rng = np.random.default_rng(3)
    n = 3000
    sa, sb = rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32)
    pa = np.where(rng.random(n) < 0.3, rng.choice(edge, n), rng.integers(1, L + 1, n))
    pb = np.where(rng.random(n) < 0.3, rng.choice(edge, n), np.clip(pa + rng.integers(-2 ** 26, 2 ** 26, n), 1, L))
    pairs = (sa, pa, sb, pb)
    recs = _records(sizes, tables, step)
    for max_span in (0, 2 ** 32 + 5):
        want = _want(pairs, sizes, tables, step, max_span, 8, recs)
        assert len(want[3]) == 3 * 8192 and want[0].tolist() == [0, 8192, 16384] and want[2][0] > 1000 and (want[2][2] > 100) == (max_span > 0)
        _set_form(monkeypatch, form)
        _same(_run(sizes, tables, step, max_span, [pairs], 8, recs), want)


# ---- records ---------------------------------------------------------------------------------------------------------------------------------
def _pairs_for_depth(D, step):
    """Pairs on one + scaffold of len(D) cells whose depth is D: D[c] pairs from cell c to cell c + 1."""
    c = np.repeat(np.arange(len(D), dtype=np.int64), np.asarray(D, np.int64))
    assert len(D) and D[-1] == 0
    return (np.zeros(len(c), np.int32), c * step + 1, np.zeros(len(c), np.int32), (c + 1) * step + 1)


@pytest.mark.parametrize("form", ["default", "plain"])
def test_records_of_every_length_and_equal_ratios(form, monkeypatch):
    """A periodic depth 4, 4, 1: every third slot has the same lowest ratio, so the first slot of the record must win - inside
    a lane, between the lanes of the wave and between their strides."""
    D = np.array([4, 4, 1] * 100 + [0], np.int64)
    step = 7
    sizes = np.array([len(D) * step - 3, 50], np.int64)
    tables = lref.identity(sizes)
    pairs = _pairs_for_depth(D, step)
    m = len(D)
    recs = [(lo, lo + n - 1, 0, m) for n in (1, 63, 64, 65, 129) for lo in (0, 2, 3, 64, 100)]
    recs += [(0, m - 1, 0, m), (m - 40, m - 1, 0, m), (0, 0, 0, m), (m - 1, m - 1, 0, m), (m, m + 7, m, m + 8)]
    for flank in (1, 2, 8, 64):
        want = _want(pairs, sizes, tables, step, 0, flank, recs)
        assert want[3][:m].tolist() == D.tolist()
        got_slots = want[1][:, 0]
        # the winner is the first slot of lowest ratio, not the last one: the whole-scaffold record picks near its left end
        assert want[1][-5][0] == flank + (2 - flank) % 3 and (got_slots >= 0).sum() >= 15    # the first slot of depth 1 with room for its left flank
        assert want[1][-1][0] == -1 and want[1][-2][0] == -1 and want[1][-3][0] == -1            # flanks cut by either end; a silent sequence
        _set_form(monkeypatch, form)
        _same(_run(sizes, tables, step, 0, [pairs], flank, recs), want)


@pytest.mark.parametrize("form", ["default", "plain"])
def test_flanks_cut_by_the_sequence_ends_and_flanks_without_pairs(form, monkeypatch):
    #            a silent stretch in the middle: slots whose left or right flank sums to 0 do not compete
    D = np.array([3, 5, 2, 6, 0, 0, 0, 4, 7, 1, 9, 0], np.int64)
    sizes = np.array([len(D) * 10, len(D) * 10], np.int64)
    tables = lref.layout([[(0, "+")], [(1, "-")]], sizes, 0)
    one = _pairs_for_depth(D, 10)
    pairs = tuple(np.concatenate([a, b]) for a, b in zip(one, (one[0] + 1, one[1], one[2] + 1, one[3])))       # the same on the reversed one
    m = len(D)
    recs = [(c, c, 0, m) for c in range(m)] + [(c, c, m, 2 * m) for c in range(m, 2 * m)] + [(0, m - 1, 0, m), (m, 2 * m - 1, m, 2 * m)]
    for flank in (1, 2, 3, 5, 6):
        want = _want(pairs, sizes, tables, 10, 0, flank, recs)
        assert want[3][:m].tolist() == D.tolist() and want[3][m:].tolist() == D[:-1][::-1].tolist() + [0]
        competing = [c for c in range(m) if want[1][c][0] >= 0]
        if flank == 1:
            assert competing == [1, 2, 8, 9]                                    # not 0 (no left flank), 3 .. 7 (a flank of 0), 10 (the terminator in the flank)
        if flank == 2:
            assert competing == [2, 5, 8]                                       # 5: depth 0 between two flanks that hold pairs
        if flank >= 5:
            assert competing == ([5] if flank == 5 else [])
        _set_form(monkeypatch, form)
        _same(_run(sizes, tables, 10, 0, [pairs], flank, recs), want)


# ---- misuse --------------------------------------------------------------------------------------------------------------------------------------
def test_misuse_leaves_the_matrix_and_an_open_map_build_as_they_were(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    _names, sizes = _scaffolds()
    tables = _tables(100, True)
    pairs = _pool()
    half = COUNTS[-1] // 2
    recs, want = _want_pool(COUNTS[-1], 100, True, 0)
    R = bref.R
    map_want = bref.build(pairs, sizes, R)
    held = np.arange(25, dtype=np.float64).reshape(5, 5)
    held = held + held.T

    def refused(call, code=EINVAL, word=None):
        with pytest.raises(_lib.HicmiError) as exc:
            call()
        assert "error %d:" % code in str(exc.value) and (word is None or word in str(exc.value)), str(exc.value)

    def changed(arr, at, value):
        out = np.array(arr)
        out[at] = value
        return out

    def untouched(ctx):
        assert ctx.n == 5 and ctx.contacts_host().tobytes() == held.tobytes()
        assert np.array_equal(ctx.row_sums()[0], held.sum(axis=1))

    sa, pa, sb, pb = pairs
    m = len(want[3])
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held)
        ctx.map_begin(sizes, R)                                               # a map build stays open through all of this
        ctx.map_add_pairs(*_first(pairs, half))
        refused(lambda: ctx.span_finish(FLANK, recs), word="without")
        refused(lambda: ctx.span_add_pairs(*pairs), word="without")
        refused(lambda: ctx.span_begin(sizes, *tables, 0), word="step")
        refused(lambda: ctx.span_begin(sizes, *tables, STEP, -1), word="max_span")
        refused(lambda: ctx.span_begin(sizes, changed(tables[0], 7, 99), *tables[1:], STEP), word="scaffold 7 ")
        refused(lambda: ctx.span_begin(sizes, tables[0], changed(tables[1], 4, tables[1][17]), *tables[2:], STEP), word="overlap")
        refused(lambda: ctx.span_finish(FLANK, recs), word="without")       # none of them opened a build
        cell_first = ctx.span_begin(sizes, *tables, STEP)
        assert cell_first.tolist() == want[0].tolist()
        ctx.span_add_pairs(*_first(pairs, 1000))
        refused(lambda: ctx.span_begin(sizes, *tables, 0))                    # a refused begin leaves the open build open
        refused(lambda: ctx.span_add_pairs(changed(sa, 200, len(sizes)), pa, sb, pb))
        refused(lambda: ctx.span_add_pairs(sa, pa, sb, changed(pb, 100, sizes[sb[100]] + 1)))
        refused(lambda: ctx.span_add_pairs(sa, changed(pa, 4000, 0), sb, pb))
        for flank in (0, -1, 4097):
            refused(lambda: ctx.span_finish(flank, recs), word="flank")
        q0, q1 = int(recs[0][2]), int(recs[0][3])
        for bad in ((q0, q1, q0, q1), (q0 - 1, q0, q0, q1), (q0 + 5, q0 + 4, q0, q1), (q0, q0, q0, q1 - 1), (q0 + 1, q0 + 1, q0 + 1, q1),
                    (0, 0, 0, m), (m, m, m, m + 1), (-1, -1, -1, 0)):
            refused(lambda: ctx.span_finish(FLANK, np.concatenate([recs[:3], [bad]])), word="record 3 ")
        untouched(ctx)
        ctx.span_add_pairs(*tuple(a[1000:] for a in pairs))                   # the build is still open, and right
        got = ctx.span_finish(FLANK, recs)
        _same((cell_first,) + got, want)
        refused(lambda: ctx.span_finish(FLANK, recs), word="without")       # ... and closed now
        # a begin gives an open span build up
        ctx.span_begin(sizes, *tables, STEP)
        ctx.span_add_pairs(*pairs)
        ctx.span_begin(sizes, *tables, STEP)
        ctx.span_add_pairs(*pairs)
        _same((cell_first,) + ctx.span_finish(FLANK, recs), want)
        untouched(ctx)
        # the map build that was open all the while takes the rest of its pairs and is what it would have been
        ctx.map_add_pairs(*tuple(a[half:] for a in pairs))
        assert ctx.map_finish() == COUNTS[-1] and ctx.contacts_host().tobytes() == map_want.tobytes()
    ctx = _lib.Context(0)                                                     # a context destroyed between begin and finish
    ctx.span_begin(sizes, *tables, STEP)
    ctx.span_add_pairs(*pairs)
    ctx.close()


# ---- the one-pass driver -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _odd_file():
    names, sizes = _scaffolds()
    data = bref.odd_file_bytes(names, sizes, 5000, seed=23)
    pairs, stats, _after = bref.parse_text(data, names, sizes)
    tables = _tables(100, True)
    # the file's scaffolds are drawn at random: give the depth something to count with pairs inside the chromosomes
    more = ref.pair_file_bytes(names, _pool())
    pairs = tuple(np.concatenate([a, b]) for a, b in zip(pairs, _pool()))
    recs = _records(sizes, tables, STEP)
    return data + b"\n" + more, (stats[0] + COUNTS[-1], stats[1] + COUNTS[-1], stats[2], stats[3]), tables, recs, \
        _want(pairs, sizes, tables, STEP, 0, FLANK, recs), pairs


def _write(tmp_path, data):
    path = str(tmp_path / "pairs.allValidPairs")
    with open(path, "wb") as fh:
        fh.write(data)
    return path


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("chunk", ["512", None])
def test_span_file_equals_the_array_calls(chunk, threads, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, stats, tables, recs, want, pairs = _odd_file()
    path = _write(tmp_path, data)
    _set_form(monkeypatch, form)
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held + held.T)
        got_stats, cell_first, picks, counters, depth = _lib.span_file(path, names, sizes, *tables, STEP, 0, FLANK, recs, ctx, threads=threads)
        assert got_stats[:4] == stats and got_stats[4] == (-(-stats[1] // 512) if chunk else 1) and stats[1] > 4 * 512
        _same((cell_first, picks, counters, depth), want)
        assert int(counters[4]) > 500 and int(counters.sum()) == stats[1]
        assert _lib.span_file(path, names, sizes, *tables, STEP, 0, FLANK, recs, ctx, threads=threads, want_depth=False)[4] is None
        assert ctx.n == 4 and ctx.contacts_host().tobytes() == (held + held.T).tobytes()
        with pytest.raises(_lib.HicmiError):
            ctx.span_finish(FLANK, recs)                                      # no build is left open
    _same(_run(sizes, tables, STEP, 0, [pairs], FLANK, recs), want)           # the array calls on the file's pairs


@pytest.mark.parametrize("chunk", ["512", None])
def test_span_file_error_writes_no_output(chunk, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, _stats, tables, recs, want, _pairs = _odd_file()
    _set_form(monkeypatch, "default")
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    lib = _lib.load()
    blob, off = _lib._name_blob(names)
    size, seq, loff, rev, seq_size = _lib._lift_tables(sizes, *tables)
    rec = np.ascontiguousarray(recs, np.int64)
    m = len(want[3])

    def call(ctx, path, flank=FLANK, rec=rec, step=STEP):
        outs = [np.full(5, -7, np.int64), np.full((len(rec), 4), -7, np.int64), np.full(5, 77, np.uint64), np.full(m, 77, np.uint64),
                np.full(len(size), -7, np.int64)]
        n_cells = ctypes.c_int64(-7)
        rc = lib.hicmi_span_file(os.fsencode(path), blob, _lib._ptr(off), len(names), _lib._ptr(size), _lib._ptr(seq), _lib._ptr(loff),
                                 _lib._ptr(rev), _lib._ptr(seq_size), len(seq_size), step, 0, flank, _lib._ptr(rec), len(rec), ctx._h, 2,
                                 _lib._ptr(outs[0]), _lib._ptr(outs[1]), _lib._ptr(outs[2]), _lib._ptr(outs[3]), _lib._ptr(outs[4]),
                                 ctypes.byref(n_cells))
        return rc, outs, n_cells.value, lib.hicmi_last_error().decode()

    def unwritten(outs, n_cells):
        return n_cells == -7 and all((o == -7).all() for o in (outs[0], outs[1], outs[4])) and all((o == 77).all() for o in outs[2:4])

    assert data.endswith(b"\n")
    bad = _write(tmp_path, data + b"read\tscaffold_4\t12x\t+\tscaffold_4\t5\n")
    with _lib.Context(0) as ctx:
        rc, outs, n_cells, message = call(ctx, bad)
        assert rc == EINVAL and message.endswith("at byte %d" % len(data)) and unwritten(outs, n_cells)
        with pytest.raises(_lib.HicmiError):
            ctx.span_finish(FLANK, recs)                                      # no build is left open
        good = _write(tmp_path, data)
        for kwargs in ({"flank": 0}, {"flank": 4097}, {"step": 0}, {"rec": np.array([[0, m, 0, m]], np.int64)}):
            rc, outs, n_cells, message = call(ctx, good, **kwargs)
            assert rc == EINVAL and unwritten(outs, n_cells), message
        rc, outs, n_cells, message = call(ctx, str(tmp_path / "missing"))
        assert rc == EINVAL and "cannot open" in message and unwritten(outs, n_cells)
        rc, outs, n_cells, message = call(ctx, good)
        assert rc == 0 and n_cells == m
        _same((outs[4], outs[1], outs[2], outs[3]), want)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip_on_the_planted_misjoin(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import _lib, supportSpans
    import test_spans_cpu as cpu
    _set_form(monkeypatch, "default")
    cfg, order, save, _paths = cpu._planted_files(tmp_path)
    cuts, full = str(tmp_path / "cuts.tsv"), str(tmp_path / "full")
    supportSpans.main(["-config", cfg, "-order", order, "-step", "1000", "-cuts", cuts, "-full", full, "-threads", "3"])
    assert "SPANS: 1 scaffold(s) suspect, 1 of 12 junction(s) weak" in capsys.readouterr().out

    def read(path):
        with open(path) as fh:
            return fh.read()

    report = read(os.path.join(save, "spanSupport.txt"))
    cpu.check_planted_report(report, read(cuts), read(os.path.join(full, "spans.depth.tsv")))
    # a context of the caller's, driven through the array calls, writes the same bytes
    out2 = str(tmp_path / "again.txt")
    with _lib.Context(0) as ctx:
        supportSpans.main(["-config", cfg, "-order", order, "-step", "1000", "-out", out2], context=ctx)
    assert read(out2) == report
    # -scaffolds on the same file equals the report on the fake context
    own, fake_own = str(tmp_path / "own.txt"), str(tmp_path / "fake_own.txt")
    supportSpans.main(["-config", cfg, "-scaffolds", "-step", "1000", "-flank", "5", "-out", own, "-cuts", cuts])
    supportSpans.main(["-config", cfg, "-scaffolds", "-step", "1000", "-flank", "5", "-out", fake_own], context=cpu.FakeContext())
    P = cpu._planted()[0]
    assert read(own) == read(fake_own) and read(cuts).split("\t")[:2] == [P["names"][P["glued"]], str(P["glue_at"])]
