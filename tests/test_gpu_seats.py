"""Seat support on the device (hicmi_seats_resident) against tests/seats_reference.py, for HICMI_SEATS_PLAIN
unset, =1 and =0, and where the store's order matters under HICMI_PAIRS_PLAIN 0 and 1.  Blocks, table and counters are
integers, so every comparison is exact: there are no tolerances."""
import ctypes
import functools
import os

import numpy as np
import pytest

import anchor_reference as aref
import buildmap_reference as bref
import ends_reference as eref
import liftmap_reference as lref
import pairs_reference as pref
import seats_reference as ref
import span_reference as sref
import test_gpu_ends as ge
from test_gpu_ends import CHROMS

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -5
# Both count forms give the same bits by design: these tests hold each to the reference but cannot tell which kernel ran; that
# the switch is read per call is checked from the source in tests/test_seats_cpu.py.
FORMS = {"default": {}, "plain": {"HICMI_SEATS_PLAIN": "1"}, "combine": {"HICMI_SEATS_PLAIN": "0"}}
FORM_NAMES = ["default", "plain", "combine"]
SLICE, SLOT_BITS, SLOTS, PROBES = (ge._constant(k) for k in ("SEATS_SLICE", "SEATS_SLOT_BITS", "SEATS_SLOTS", "SEATS_PROBES"))
COUNTS = [1, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 5000]
WINDOW = 500
# the three chromosomes of test_gpu_ends and a fourth of one scaffold
FOUR = CHROMS + [[(30, "+")]]


def _set_form(monkeypatch, form, store=None):
    for key in ("HICMI_SEATS_PLAIN", "HICMI_PAIRS_PLAIN", "HICMI_PAIRS_FIRST_PAIRS", "HICMI_ENDS_PLAIN", "HICMI_ANCHOR_PLAIN", "HICMI_SPANS_PLAIN",
                "HICMI_BUILDMAP_CHUNK_PAIRS", "HICMI_BUILDMAP_PLAIN", "HICMI_LIFTMAP_PLAIN"):
        monkeypatch.delenv(key, raising=False)
    for key, value in FORMS[form].items():
        monkeypatch.setenv(key, value)
    if store is not None:
        monkeypatch.setenv("HICMI_PAIRS_PLAIN", store)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


_scaffolds = ge._scaffolds


@functools.lru_cache(maxsize=None)
def _tables(gap=100):
    _names, sizes = _scaffolds()
    return _frozen(*lref.layout(FOUR, sizes, gap, drop_unplaced=True))


@functools.lru_cache(maxsize=None)
def _pool():
    """5,000 pairs, most of them between two placed scaffolds, of one chromosome or of two; the first and last bases, both
    edges of both zones at the window 500 and the two bases at a half's edge favoured; some on one scaffold, some with an
    end on a dropped scaffold."""
    _names, sizes = _scaffolds()
    rng = np.random.default_rng(11)
    n = COUNTS[-1]
    members = [np.array([s for s, _o in ch]) for ch in FOUR]
    placed = np.concatenate(members)
    dropped = np.setdiff1d(np.arange(40), placed)
    ch = rng.integers(0, 3, n)
    sa = np.array([rng.choice(members[c]) for c in ch])
    sb = np.array([rng.choice(members[c]) for c in ch])

    def positions(s):
        L = sizes[s]
        p = 1 + np.floor(rng.random(n) * L).astype(np.int64)
        edge = rng.integers(0, 12, n)
        zone = np.minimum(WINDOW, L // 2)
        out = np.select([edge == 0, edge == 1, edge == 2, edge == 3, edge == 4, edge == 5, edge == 6, edge == 7],
                        [np.ones(n, np.int64), L, np.maximum(zone, 1), np.minimum(zone + 1, L), np.maximum(L - zone, 1), np.minimum(L - zone + 1, L),
                         L - L // 2, np.minimum(L - L // 2 + 1, L)], p)
        return out.astype(np.int64)

    kind = rng.integers(0, 20, n)
    trans = kind <= 3
    sb[trans] = rng.choice(placed, trans.sum())
    same = (kind == 4) | (kind == 5)
    sb[same] = sa[same]
    lost = (kind == 6) | (kind == 7)
    sb[lost] = rng.choice(dropped, lost.sum())
    pa, pb = positions(sa), positions(sb)
    swap = rng.random(n) < 0.5
    sa, sb = np.where(swap, sb, sa), np.where(swap, sa, sb)
    pa, pb = np.where(swap, pb, pa), np.where(swap, pa, pb)
    return _frozen(sa.astype(np.int32), pa.astype(np.int64), sb.astype(np.int32), pb.astype(np.int64))


def _first(pairs, n):
    return tuple(a[:n] for a in pairs)


def _want(pairs, sizes, tables, window):
    T, counters = ref.store_table(pref.keep(pairs), pref.intra(pairs, len(sizes)), sizes, tables, window)
    first, n = ref.number_blocks(sizes, tables)
    assert T.shape == (n,) and int(counters.sum()) == len(pairs[0])
    return first, T, counters


@functools.lru_cache(maxsize=None)
def _want_pool(n, window, gap=100):
    _names, sizes = _scaffolds()
    return _want(_first(_pool(), n), sizes, _tables(gap), window)


def _load(ctx, sizes, parts):
    ctx.pairs_begin(sizes)
    for p in parts:
        ctx.pairs_add(*p)


def _run(sizes, tables, window, parts, ctx=None):
    from hic_genome_assembler_amd import _lib
    if ctx is None:
        with _lib.Context(0) as own:
            return _run(sizes, tables, window, parts, own)
    _load(ctx, sizes, parts)
    try:
        return ctx.seats_resident(sizes, *tables, window)
    finally:
        ctx.pairs_drop()


def _same(got, want):
    first, T, counters = want
    assert got[0].dtype == np.int64 and got[0].tolist() == first.tolist()
    assert got[1].dtype == np.uint64 and got[1].shape == T.shape and got[1].tobytes() == T.tobytes()
    assert got[2].dtype == np.uint64 and got[2].shape == (5,) and got[2].tolist() == counters.tolist()


# ---- the pool, pair counts, windows ---------------------------------------------------------------------------------------------------
def test_the_pool_holds_what_it_should():
    _names, sizes = _scaffolds()
    pairs, tables = _pool(), _tables()
    n_seq = len(tables[3])
    seated, middle, trans, same, unlifted = ref.table(pairs, sizes, tables, WINDOW)[1].tolist()
    assert min(seated, middle, trans, same, unlifted) >= 100, (seated, middle, trans, same, unlifted)
    _kind, index = ref.classify(pairs, sizes, tables, WINDOW)
    first, _n = ref.number_blocks(sizes, tables)
    starts = np.sort(first[first >= 0])
    gaps = index[:, 2:][index[:, 2:] >= 0]
    inside = gaps - starts[np.searchsorted(starts, gaps, side="right") - 1] - n_seq
    assert (inside >= 0).all() and (np.bincount(inside % 4, minlength=4) >= 100).all(), np.bincount(inside % 4, minlength=4)
    sa, pa, sb, pb = pairs
    for s, p in ((sa, pa), (sb, pb)):
        L = sizes[s]
        assert (p == 1).any() and (p == L).any() and ((L == 1) & (tables[0][s] >= 0)).any()
        for size in (999, 1000, 3007, 70000):
            half = size - size // 2
            zone = min(WINDOW, size // 2)
            at = p[L == size]
            assert all((at == x).any() for x in (half, half + 1, zone, zone + 1, size - zone, size - zone + 1)), size
    assert ref.table(pairs, sizes, tables, 10 ** 6)[1][ref.MIDDLE] == 0 and ref.table(pairs, sizes, tables, 1)[1][ref.MIDDLE] > middle


@pytest.mark.parametrize("form", FORM_NAMES)
def test_pair_counts_at_the_wave_workgroup_and_slice_edges(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        for n in COUNTS:
            _same(_run(sizes, _tables(), WINDOW, [_first(_pool(), n)], ctx), _want_pool(n, WINDOW))


@pytest.mark.parametrize("form", FORM_NAMES)
def test_windows_gaps_and_the_five_counters(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        _load(ctx, sizes, [_pool()])                                          # one store, counted again and again
        for gap in (0, 100):
            for window in (1, 500, 10 ** 6):
                _same(ctx.seats_resident(sizes, *_tables(gap), window), _want_pool(COUNTS[-1], window, gap))
        assert _want_pool(COUNTS[-1], 500, 0)[1].tobytes() == _want_pool(COUNTS[-1], 500, 100)[1].tobytes()      # the gaps play no part
        assert _want_pool(COUNTS[-1], 1)[1].tobytes() != _want_pool(COUNTS[-1], 500)[1].tobytes()


# ---- the table in LDS --------------------------------------------------------------------------------------------------------------------
def _replay_spills(index):
    """The adds of one slice that find no room in the table of the combining kernel, taken in index order: the hash and the
    probe rule of seats_add_lds in NumPy integers."""
    keys = np.full(SLOTS, -1, np.int64)
    spilled = 0
    for k in index.tolist():
        h = ((k * 0x9E3779B9) & 0xFFFFFFFF) >> (32 - SLOT_BITS)
        for _probe in range(PROBES):
            if keys[h] in (-1, k):
                keys[h] = k
                break
            h = (h + 1) & (SLOTS - 1)
        else:
            spilled += 1
    return spilled


@functools.lru_cache(maxsize=None)
def _crowded():
    """One chromosome of sixty scaffolds of 1,000 bases at a huge window: 60 x (1 + 240) counters, the scaffolds and positions
    of every pair drawn uniformly, so that the first slice alone holds more distinct counters than the table has slots."""
    rng = np.random.default_rng(17)
    sizes = np.full(60, 1000, np.int64)
    tables = lref.layout([[(s, "+-"[s % 2]) for s in range(60)]], sizes, 100, drop_unplaced=True)
    n = 2 * SLICE + 300
    sa = rng.integers(0, 60, n)
    sb = (sa + rng.integers(1, 60, n)) % 60
    pa, pb = rng.integers(1, 1001, n), rng.integers(1, 1001, n)
    return _frozen(sizes) + (_frozen(*tables), _frozen(sa.astype(np.int32), pa.astype(np.int64), sb.astype(np.int32), pb.astype(np.int64)))


@pytest.mark.parametrize("form", FORM_NAMES)
def test_a_slice_with_more_counters_than_the_probes_can_place(form, monkeypatch):
    sizes, tables, pairs = _crowded()
    kind, index = ref.classify(_first(pairs, SLICE), sizes, tables, 10 ** 6)
    first_slice = index[index >= 0]
    # whatever order the lanes arrive in, a table of SLOTS slots cannot hold more distinct counters than that; taken in
    # index order, the replay of the probe rule says how many adds it turns away
    assert (kind == ref.SEATED).all() and len(first_slice) == 4 * SLICE
    assert len(np.unique(first_slice)) > SLOTS and _replay_spills(first_slice) >= 1
    want = _want(pairs, sizes, tables, 10 ** 6)
    assert want[2].tolist() == [len(pairs[0]), 0, 0, 0, 0] and int(want[1].sum()) == 4 * len(pairs[0])
    _set_form(monkeypatch, form)
    _same(_run(sizes, tables, 10 ** 6, [pairs]), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_slices_whose_pairs_are_all_one_pair(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    tables = _tables()
    _set_form(monkeypatch, form)
    # base 3,000 of scaffold 4 (3,007 bases, reversed: its second half, and as it lies its LEFT zone) and base 5 of scaffold 3,
    # which lies first in Chr_1 (its first half, its LEFT zone): two chromosome counters and two gap counters
    with _lib.Context(0) as ctx:
        for n in (SLICE, 3 * SLICE + 5):
            pairs = tuple(np.full(n, v, dtype=t) for v, t in ((4, np.int32), (3000, np.int64), (3, np.int32), (5, np.int64)))
            want = _want(pairs, sizes, tables, WINDOW)
            at = np.flatnonzero(want[1]).tolist()
            assert want[2].tolist() == [n, 0, 0, 0, 0] and len(at) == 4 and want[1][at].tolist() == [n] * 4
            got = _run(sizes, tables, WINDOW, [pairs], ctx)
            _same(got, want)
            assert got[1][at].tolist() == [n] * 4 and int(got[1].sum()) == 4 * n


@pytest.mark.parametrize("form", FORM_NAMES)
def test_scaffolds_of_2_to_the_33_and_positions_above_2_to_the_32(form, monkeypatch):
    L = 2 ** 33
    sizes = np.array([L, L + 1, L, 5], dtype=np.int64)
    tables = lref.layout([[(0, "+"), (1, "-"), (2, "+")]], sizes, 100, drop_unplaced=True)
    _set_form(monkeypatch, form)
    for window in (2 ** 20, 2 ** 32 + 1):
        mid = L // 2
        edge = [1, window, window + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, mid, mid + 1, mid + 2, L - window, L - window + 1, L]
        ends = [(s, p) for s in range(3) for p in edge] + [(1, L + 1), (3, 1), (3, 5)]
        rows = [a + b for a in ends for b in ends]
        pairs = tuple(np.array(col, dtype=t) for col, t in zip(zip(*rows), (np.int32, np.int64, np.int32, np.int64)))
        want = _want(pairs, sizes, tables, window)
        assert want[2][ref.SEATED] > 0 and (want[2][ref.MIDDLE] > 0) == (window < 2 ** 32)      # at the larger window every base is in a zone
        _same(_run(sizes, tables, window, [pairs]), want)


# ---- the order of the store plays no part -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["0", "1"])
@pytest.mark.parametrize("form", FORM_NAMES)
def test_any_chunking_and_any_order_give_the_same_bits(form, store, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    want = _want_pool(COUNTS[-1], WINDOW)
    pairs = _pool()
    n = COUNTS[-1]
    _set_form(monkeypatch, form, store)
    with _lib.Context(0) as ctx:
        cuts = [0, 1, 258, n]
        parts = [tuple(a[lo:hi] for a in pairs) for lo, hi in zip(cuts, cuts[1:])]
        assert [len(p[0]) for p in parts][:2] == [1, 257]
        _same(_run(sizes, _tables(), WINDOW, parts, ctx), want)
        _same(_run(sizes, _tables(), WINDOW, [tuple(a[::-1] for a in pairs)], ctx), want)
        swapped = (pairs[2], pairs[3], pairs[0], pairs[1])                    # the mates of every pair exchanged
        _same(_run(sizes, _tables(), WINDOW, [swapped], ctx), want)
        monkeypatch.setenv("HICMI_PAIRS_FIRST_PAIRS", "256")                  # a store that grows several times while it is loaded
        _same(_run(sizes, _tables(), WINDOW, [tuple(a[lo:lo + 700] for a in pairs) for lo in range(0, n, 700)], ctx), want)


# ---- the equivalence on the device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
def test_a_block_is_what_anchor_resident_counts_on_the_layout_without_its_scaffold(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    tables, pairs = _tables(), _pool()
    n_seq = len(tables[3])
    _set_form(monkeypatch, form)
    # a chromosome's first, its last, a middle one, one of a single base, and the only scaffold of a chromosome
    chosen = [3, 7, 17, 5, 30]
    assert [int(sizes[c]) for c in chosen] == [70000, 1000, 70000, 1, 1] and FOUR[0][0][0] == 3 and FOUR[0][-1][0] == 7 and FOUR[3] == [(30, "+")]
    with _lib.Context(0) as ctx:
        _load(ctx, sizes, [pairs])
        first, T, _counters = ctx.seats_resident(sizes, *tables, WINDOW)
        for c in chosen:
            q = int(tables[0][c])
            a, gaps, k_c = ref.own_block(T, first, sizes, tables, c)
            assert not gaps[k_c].any()
            less = lref.layout([[(s, o) for s, o in chrom if s != c] for chrom in FOUR], sizes, 100, drop_unplaced=True)
            first1, T1, _c1 = ctx.anchor_resident(sizes, *less, None, WINDOW)
            assert T1[first1[c]:first1[c] + n_seq].tobytes() == a.tobytes() and (a.sum() > 0 or c == 30)
            if len(gaps) > 1:
                target = np.full(40, -1, np.int32)
                target[c] = q
                _first2, T2, _c2 = ctx.anchor_resident(sizes, *less, target, WINDOW)
                assert T2.tobytes() == np.delete(gaps, k_c, axis=0).reshape(-1).tobytes() and T2.sum() > 0
            else:
                assert c == 30


# ---- repeat calls -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["0", "1"])
@pytest.mark.parametrize("form", FORM_NAMES)
def test_three_calls_with_a_scaffold_moved_between_them_leave_the_store_unchanged(form, store, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    pairs = _pool()
    _set_form(monkeypatch, form, store)
    with _lib.Context(0) as ctx:
        _load(ctx, sizes, [pairs])
        before = ctx.pairs_fetch()
        chroms = [list(ch) for ch in FOUR]
        seen = set()
        for move in (None, (0, 1, 5), (1, 6, 0)):
            if move:
                q, i, j = move
                chroms[q].insert(j, chroms[q].pop(i))
            tables = lref.layout(chroms, sizes, 100, drop_unplaced=True)
            got = ctx.seats_resident(sizes, *tables, WINDOW)
            _same(got, _want(pairs, sizes, tables, WINDOW))
            seen.add(got[1].tobytes())
        assert len(seen) == 3                                                    # the moves moved counts
        after = ctx.pairs_fetch()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        assert ctx.pairs_info()[0] == int(pref.mask(pairs).sum())


# ---- misuse --------------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, sizes, tables, window, n_table, null=None):
    """hicmi_seats_resident called raw on outputs filled with marks: (rc, table, counters, first, n_out, message)."""
    from hic_genome_assembler_amd import _lib
    lib = _lib.load()
    size, seq, loff, rev, seq_size = _lib._lift_tables(sizes, *tables)
    table, counters, first = np.full(n_table, 77, np.uint64), np.full(5, 77, np.uint64), np.full(len(size), -7, np.int64)
    n_out = ctypes.c_int64(-7)
    outs = [_lib._ptr(table), _lib._ptr(counters), _lib._ptr(first), ctypes.byref(n_out)]
    if null is not None:
        outs[null] = None
    rc = lib.hicmi_seats_resident(ctx._h, _lib._ptr(size), len(size), _lib._ptr(seq), _lib._ptr(loff), _lib._ptr(rev), _lib._ptr(seq_size),
                                  len(seq_size), window, *outs)
    return rc, table, counters, first, n_out.value, lib.hicmi_last_error().decode()


def _unwritten(got):
    _rc, table, counters, first, n_out, _message = got
    return n_out == -7 and (table == 77).all() and (counters == 77).all() and (first == -7).all()


def test_misuse_returns_einval_writes_nothing_and_leaves_the_matrix_and_the_open_builds_as_they_were(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    _names, sizes = _scaffolds()
    tables, pairs = _tables(), _pool()
    S, n = len(sizes), COUNTS[-1]
    half = n // 2
    want = _want_pool(n, WINDOW)
    n_table = len(want[1])
    target = np.full(S, -1, np.int32)
    target[10] = 0
    map_want = bref.build(pairs, sizes, bref.R)
    span_recs = [(0, 10, 0, int(sref.number_cells(sizes, tables, 500)[1][1]))]
    span_D, span_counters, _marks = sref.depth(pairs, sizes, tables, 500)
    span_picks = sref.picks(span_D, 3, span_recs)
    ends_T, ends_counters = eref.table(pairs, sizes, tables, WINDOW, 2)
    anchor_T, anchor_counters = aref.table(pairs, sizes, tables, target, WINDOW)
    held = np.arange(25, dtype=np.float64).reshape(5, 5)
    held = held + held.T
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held)
        ctx.map_begin(sizes, bref.R)                                          # a map, a span, an ends and an anchor build stay open
        ctx.map_add_pairs(*_first(pairs, half))
        ctx.span_begin(sizes, *tables, 500)
        ctx.span_add_pairs(*_first(pairs, half))
        ctx.ends_begin(sizes, *tables, WINDOW, 2)
        ctx.ends_add_pairs(*_first(pairs, half))
        ctx.anchor_begin(sizes, *tables, target, WINDOW)
        ctx.anchor_add_pairs(*_first(pairs, half))
        got = _raw(ctx, sizes, tables, WINDOW, n_table)
        assert got[0] == EINVAL and "hicmi_seats_resident without a pair store" in got[5] and _unwritten(got)
        _load(ctx, sizes, [pairs])
        store = ctx.pairs_fetch()
        other = np.array(sizes)
        other[3] += 1
        everything_dropped = (np.full(S, -1, np.int32),) + tuple(tables[1:])
        for got, word in ((_raw(ctx, other, tables, WINDOW, n_table), "sizes"),
                          (_raw(ctx, sizes[:-1], (tables[0][:-1], tables[1][:-1], tables[2][:-1], tables[3]), WINDOW, n_table), "sizes"),
                          (_raw(ctx, sizes, tables, 0, n_table), "window 0 is below 1"),
                          (_raw(ctx, sizes, tables, -5, n_table), "window"),
                          (_raw(ctx, sizes, everything_dropped, WINDOW, n_table), "placed"),
                          (_raw(ctx, sizes, tables, WINDOW, n_table, null=0), "bad arguments"),
                          (_raw(ctx, sizes, tables, WINDOW, n_table, null=1), "bad arguments"),
                          (_raw(ctx, sizes, tables, WINDOW, n_table, null=2), "bad arguments"),
                          (_raw(ctx, sizes, tables, WINDOW, n_table, null=3), "bad arguments")):
            assert got[0] == EINVAL and word in got[5] and _unwritten(got), got[5]
        with pytest.raises(_lib.HicmiError) as exc:                               # tables the lift check refuses name the scaffold
            bad = np.array(tables[0])
            bad[7] = 99
            ctx.seats_resident(sizes, bad, *tables[1:], WINDOW)
        assert "error %d:" % EINVAL in str(exc.value) and "scaffold 7 " in str(exc.value)
        # the call answers while the four builds are open, and raw it returns n_table
        rc, table, counters, first, got_table, _message = _raw(ctx, sizes, tables, WINDOW, n_table)
        assert rc == 0 and got_table == n_table
        _same((first, table, counters), want)
        _same(ctx.seats_resident(sizes, *tables, WINDOW), want)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(store, ctx.pairs_fetch()))
        assert ctx.n == 5 and ctx.contacts_host().tobytes() == held.tobytes() and np.array_equal(ctx.row_sums()[0], held.sum(axis=1))
        # the builds that were open all the while take the rest of their pairs and are what they would have been
        ctx.anchor_add_pairs(*tuple(a[half:] for a in pairs))
        got_T, got_counters = ctx.anchor_finish()
        assert got_T.tobytes() == anchor_T.tobytes() and got_counters.tolist() == anchor_counters.tolist()
        ctx.ends_add_pairs(*tuple(a[half:] for a in pairs))
        got_T, got_counters = ctx.ends_finish()
        assert got_T.tobytes() == ends_T.tobytes() and got_counters.tolist() == ends_counters.tolist()
        ctx.span_add_pairs(*tuple(a[half:] for a in pairs))
        picks, counters, depth = ctx.span_finish(3, span_recs)
        assert depth.tobytes() == span_D.tobytes() and counters.tolist() == span_counters.tolist() and picks.tolist() == span_picks.tolist()
        ctx.map_add_pairs(*tuple(a[half:] for a in pairs))
        assert ctx.map_finish() == n and ctx.contacts_host().tobytes() == map_want.tobytes()
        ctx.pairs_drop()
        # 5,793 scaffolds in one chromosome pass 2^27 counters - sizes only, nothing that large is allocated
        many = 5793
        ones = np.ones(many, np.int64)
        ctx.pairs_begin(ones)
        deep = lref.layout([[(s, "+") for s in range(many)]], ones, 0, drop_unplaced=True)
        got = _raw(ctx, ones, deep, 1, 8)
        assert got[0] == EUNSUPPORTED and "counters" in got[5] and _unwritten(got)


# ---- the command line ----------------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip_on_the_planted_displaced_case(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import polishOrder, supportSeats
    import test_seats_cpu as cpu
    _set_form(monkeypatch, "default")
    cfg, order, _save = cpu.displaced_files(tmp_path)
    made = {}
    for where, context in (("device", None), ("stand_in", cpu.StandInContext())):
        d = tmp_path / where
        d.mkdir()
        moved, report, full, out = str(d / "moved.txt"), str(d / "seats.txt"), str(d / "full"), str(d / "polished")
        supportSeats.main(["-config", cfg, "-order", order, "-window", "5000", "-moved", moved, "-out", report, "-full", full, "-threads", "3"],
                          context=context)
        context = None if context is None else cpu.StandInContext()
        status, rounds, _log = polishOrder.main(["-config", cfg, "-order", order, "-window", "5000", "-moves", "flip,relocate", "-out", out],
                                                context=context)
        assert (status, rounds) == ("converged", 1)
        made[where] = [cpu._read(p) for p in (moved, report, os.path.join(full, "seats.chromosomes.tsv"), os.path.join(full, "seats.gaps.tsv"),
                                              os.path.join(out, "orders.txt"), os.path.join(out, "polish.log"),
                                              os.path.join(out, "polish_summary.tsv"))]
    assert made["device"] == made["stand_in"]
    cpu.check_displaced_outputs(made["device"][0], made["device"][4], made["device"][1])
    assert "3 relocation(s)" in capsys.readouterr().out
