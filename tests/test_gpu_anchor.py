"""Anchoring on the device (hicmi_anchor_begin / _add_pairs / _finish / _file) against
tests/anchor_reference.py, for HICMI_ANCHOR_PLAIN unset, =1 and =0, in sequence mode and in rank mode.  Blocks, table and
counters are integers, so every comparison is exact: there are no tolerances."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import anchor_reference as ref
import buildmap_reference as bref
import ends_reference as eref
import liftmap_reference as lref
import span_reference as sref
from test_gpu_ends import CHROMS

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -5
# Both count forms give the same bits by design: these tests hold each to the reference but cannot tell which kernel ran; that
# the switch is read per call is checked from the source in tests/test_anchor_cpu.py.
FORMS = {"default": {}, "plain": {"HICMI_ANCHOR_PLAIN": "1"}, "combine": {"HICMI_ANCHOR_PLAIN": "0"}}
FORM_NAMES = ["default", "plain", "combine"]
MODES = ["sequence", "rank"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    with open(os.path.join(ROOT, "hic_genome_assembler_amd", "csrc", "hicmi_internal.h")) as fh:
        text = fh.read()
    value = re.search(r"static constexpr int %s = ([^;]+);" % name, text).group(1)
    return 1 << _constant(value.split("<<")[1].strip()) if "<<" in value else int(value)


SLICE, SLOT_BITS, SLOTS, PROBES = (_constant(k) for k in ("ANCHOR_SLICE", "ANCHOR_SLOT_BITS", "ANCHOR_SLOTS", "ANCHOR_PROBES"))
COUNTS = [1, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 5000]
WINDOW = 500


def _set_form(monkeypatch, form):
    for key in ("HICMI_ANCHOR_PLAIN", "HICMI_ENDS_PLAIN", "HICMI_SPANS_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS", "HICMI_BUILDMAP_PLAIN",
                "HICMI_LIFTMAP_PLAIN"):
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
def _tables(gap=100):
    """The three chromosomes of test_gpu_ends placed, the other twenty scaffolds dropped: the candidates."""
    _names, sizes = _scaffolds()
    return _frozen(*lref.layout(CHROMS, sizes, gap, drop_unplaced=True))


@functools.lru_cache(maxsize=None)
def _target(mode):
    """Rank mode: the candidates in turn against Chr_1, Chr_2, Chr_3 and nothing, so that every size has a target."""
    if mode == "sequence":
        return None
    _names, sizes = _scaffolds()
    target = np.full(40, -1, np.int32)
    for k, c in enumerate(np.flatnonzero(_tables()[0] < 0).tolist()):
        target[c] = k % 4 - 1
    assert {int(sizes[c]) for c in np.flatnonzero(target >= 0)} == {1, 999, 1000, 1001, 3007}       # the three of 70,000 are placed
    return _frozen(target)[0]


@functools.lru_cache(maxsize=None)
def _pool():
    """5,000 pairs: most of them between a dropped scaffold and a placed one, the ends of the long scaffolds, the halves of
    the candidates and the very first and last bases favoured; some between two dropped ones, on one scaffold, or anywhere."""
    _names, sizes = _scaffolds()
    rng = np.random.default_rng(5)
    n = COUNTS[-1]
    dropped = np.flatnonzero(_tables()[0] < 0)
    placed = np.flatnonzero(_tables()[0] >= 0)
    sa, sb = rng.choice(dropped, n), rng.choice(placed, n)

    def positions(s):
        L = sizes[s]
        p = 1 + np.floor(rng.random(n) * L).astype(np.int64)
        edge = rng.integers(0, 8, n)
        near = np.minimum(rng.integers(1, 601, n), L)                  # the first or the last 600 bases, where there are that many
        near[edge >= 6] = 1                                            # ... and the very first and last base
        out = np.where(edge % 2 == 0, near, L + 1 - near)
        half = L - L // 2                                              # the last base of the first half and the first of the second
        out = np.where(edge == 2, half, np.where(edge == 3, np.minimum(half + 1, L), out))
        return np.where((edge == 4) | (edge == 5), p, out)

    pa, pb = positions(sa), positions(sb)
    kind = rng.integers(0, 12, n)
    both_dropped = kind == 0
    sb[both_dropped] = rng.choice(dropped, both_dropped.sum())
    same = kind == 1
    sb[same] = sa[same]
    both_placed = kind == 2
    sa[both_placed] = rng.choice(placed, both_placed.sum())
    redo = both_dropped | same | both_placed
    pa[redo] = (1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64))[redo]
    pb[redo] = (1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64))[redo]
    swap = rng.random(n) < 0.5                                         # either mate may be the dropped one
    sa, sb = np.where(swap, sb, sa), np.where(swap, sa, sb)
    pa, pb = np.where(swap, pb, pa), np.where(swap, pa, pb)
    return _frozen(sa.astype(np.int32), pa.astype(np.int64), sb.astype(np.int32), pb.astype(np.int64))


def test_the_pool_holds_what_it_should():
    _names, sizes = _scaffolds()
    sa, pa, sb, pb = _pool()
    seq = _tables()[0]
    for s, p in ((sa, pa), (sb, pb)):
        on = seq[s] < 0                                                # ends on candidates
        L = sizes[s]
        assert ((L[on] == 1)).any() and (p[on] == 1).any() and (p[on] == L[on]).any()
        for size in (999, 1000, 3007):                                 # both halves, at their edge, of odd and even candidates
            half = size - size // 2
            assert (p[on & (L == size)] == half).any() and (p[on & (L == size)] == half + 1).any()
    for mode in MODES:
        for window in (1, 500, 10 ** 6):
            counters = _want_pool(COUNTS[-1], mode, window)[2]
            anchored, middle, elsewhere, skipped, unplaced, placed = counters.tolist()
            assert anchored > 300 and unplaced > 300 and placed > 200
            assert (elsewhere > 300) == (skipped > 300) == (mode == "rank") and (middle > 100) == (mode == "rank" and window < 10 ** 6)


def _first(pairs, n):
    return tuple(a[:n] for a in pairs)


def _want(pairs, sizes, tables, target, window):
    T, counters = ref.table(pairs, sizes, tables, target, window)
    first, n = ref.number_blocks(sizes, tables, target)
    assert T.shape == (n,) and int(counters.sum()) == len(pairs[0]) and int(T.sum()) == int(counters[ref.ANCHORED])
    return first, T, counters


@functools.lru_cache(maxsize=None)
def _want_pool(n, mode, window):
    _names, sizes = _scaffolds()
    return _want(_first(_pool(), n), sizes, _tables(), _target(mode), window)


def _run(sizes, tables, target, window, parts, ctx=None):
    from hic_genome_assembler_amd import _lib
    if ctx is None:
        with _lib.Context(0) as own:
            return _run(sizes, tables, target, window, parts, own)
    first = ctx.anchor_begin(sizes, *tables, target, window)
    for p in parts:
        ctx.anchor_add_pairs(*p)
    return (first,) + ctx.anchor_finish()


def _same(got, want):
    first, T, counters = want
    assert got[0].dtype == np.int64 and got[0].tolist() == first.tolist()
    assert got[1].dtype == np.uint64 and got[1].shape == T.shape and got[1].tobytes() == T.tobytes()
    assert got[2].dtype == np.uint64 and got[2].tolist() == counters.tolist()


# ---- pair counts, windows, kinds of pairs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_pair_counts_at_the_wave_workgroup_and_slice_edges(mode, form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        for n in COUNTS:
            _same(_run(sizes, _tables(), _target(mode), WINDOW, [_first(_pool(), n)], ctx), _want_pool(n, mode, WINDOW))


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_windows_and_the_six_counters(mode, form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        for window in (1, 500, 10 ** 6):
            _same(_run(sizes, _tables(), _target(mode), window, [_pool()], ctx), _want_pool(COUNTS[-1], mode, window))
        for gap in (0, 100):                                                  # the gaps play no part
            tables = _tables(gap)
            _same(_run(sizes, tables, _target(mode), 500, [_pool()], ctx), _want(_pool(), sizes, tables, _target(mode), 500))


# ---- the table in LDS --------------------------------------------------------------------------------------------------------------------
def _replay_spills(index):
    """The pairs of one slice that find no room in the table of the combining kernel, taken in index order: the hash and
    the probe rule of anchor_add_lds in NumPy integers."""
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
    """Sixty candidates against a chromosome of sixty scaffolds in rank mode at a huge window: 60 x 60 x 4 counters, the
    scaffolds, halves and zones of every pair drawn uniformly, so that the first slice alone holds more distinct counters
    than the table has slots."""
    rng = np.random.default_rng(17)
    sizes = np.full(120, 1000, np.int64)
    tables = lref.layout([[(s, "+-"[s % 2]) for s in range(60)]], sizes, 100, drop_unplaced=True)
    target = np.where(np.arange(120) >= 60, 0, -1).astype(np.int32)
    n = 2 * SLICE + 300
    sa, sb = rng.integers(60, 120, n), rng.integers(0, 60, n)
    pa, pb = rng.integers(1, 1001, n), rng.integers(1, 1001, n)
    return _frozen(sizes, target) + (_frozen(*tables), _frozen(sa.astype(np.int32), pa.astype(np.int64), sb.astype(np.int32), pb.astype(np.int64)))


@pytest.mark.parametrize("form", FORM_NAMES)
def test_a_slice_with_more_counters_than_the_probes_can_place(form, monkeypatch):
    sizes, target, tables, pairs = _crowded()
    kind, index = ref.classify(_first(pairs, SLICE), sizes, tables, target, 10 ** 6)
    first_slice = index[kind == ref.ANCHORED]
    # whatever order the lanes arrive in, a table of SLOTS slots cannot hold more distinct counters than that; taken in
    # index order, the replay of the probe rule says how many pairs it turns away
    assert len(np.unique(first_slice)) > SLOTS and _replay_spills(first_slice) >= 1
    want = _want(pairs, sizes, tables, target, 10 ** 6)
    assert want[2][ref.ANCHORED] == len(pairs[0]) and want[1].max() < 20
    _set_form(monkeypatch, form)
    _same(_run(sizes, tables, target, 10 ** 6, [pairs]), want)


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_slices_whose_pairs_all_hit_one_counter(mode, form, monkeypatch):
    _names, sizes = _scaffolds()
    tables, target = _tables(), _target(mode)
    c = int(np.flatnonzero((tables[0] < 0) & (sizes == 3007) & ((target if target is not None else np.zeros(40)) == 0))[0])
    # base 2,000 of the candidate, in its second half, and base 5 of scaffold 4, which lies first in Chr_1: its LEFT zone
    for n in (SLICE, 3 * SLICE + 5):
        pairs = tuple(np.full(n, v, dtype=t) for v, t in ((c, np.int32), (2000, np.int64), (3, np.int32), (5, np.int64)))
        want = _want(pairs, sizes, tables, target, WINDOW)
        at = int(want[0][c]) + (0 if mode == "sequence" else 0 * 4 + 1 * 2 + ref.LEFT)
        assert want[2].tolist() == [n, 0, 0, 0, 0, 0] and np.flatnonzero(want[1]).tolist() == [at] and int(want[1][at]) == n
        _set_form(monkeypatch, form)
        got = _run(sizes, tables, target, WINDOW, [pairs])
        _same(got, want)
        assert int(got[1][at]) == n


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("mode", MODES)
def test_any_chunking_and_any_order_give_the_same_bits(mode, form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    want = _want_pool(COUNTS[-1], mode, WINDOW)
    pairs = _pool()
    n = COUNTS[-1]
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        for cuts in ([0, n], [0, 1, 258, n]):
            parts = [tuple(a[lo:hi] for a in pairs) for lo, hi in zip(cuts, cuts[1:])]
            assert [len(p[0]) for p in parts][:2] in ([n], [1, 257])
            _same(_run(sizes, _tables(), _target(mode), WINDOW, parts, ctx), want)
        _same(_run(sizes, _tables(), _target(mode), WINDOW, [tuple(a[::-1] for a in pairs)], ctx), want)
        swapped = (pairs[2], pairs[3], pairs[0], pairs[1])                    # the mates of every pair exchanged
        _same(_run(sizes, _tables(), _target(mode), WINDOW, [swapped], ctx), want)


# ---- misuse --------------------------------------------------------------------------------------------------------------------------------------
def test_misuse_leaves_the_matrix_and_the_open_map_span_and_ends_builds_as_they_were(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    _names, sizes = _scaffolds()
    tables, target = _tables(), _target("rank")
    pairs = _pool()
    n = COUNTS[-1]
    half = n // 2
    want = _want_pool(n, "rank", WINDOW)
    want_seq = _want_pool(n, "sequence", WINDOW)
    map_want = bref.build(pairs, sizes, bref.R)
    span_recs = [(0, 10, 0, int(sref.number_cells(sizes, tables, 500)[1][1]))]
    span_D, span_counters, _marks = sref.depth(pairs, sizes, tables, 500)
    span_picks = sref.picks(span_D, 3, span_recs)
    ends_T, ends_counters = eref.table(pairs, sizes, tables, WINDOW, 2)
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
    a_candidate = int(np.flatnonzero(target >= 0)[0])
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held)
        ctx.map_begin(sizes, bref.R)                                          # a map, a span and an ends build stay open through all of this
        ctx.map_add_pairs(*_first(pairs, half))
        ctx.span_begin(sizes, *tables, 500)
        ctx.span_add_pairs(*_first(pairs, half))
        ctx.ends_begin(sizes, *tables, WINDOW, 2)
        ctx.ends_add_pairs(*_first(pairs, half))
        refused(lambda: ctx.anchor_finish(), word="without")
        refused(lambda: ctx.anchor_add_pairs(*pairs), word="without")
        for tgt in (None, target):
            refused(lambda: ctx.anchor_begin(sizes, *tables, tgt, 0), word="window")
            refused(lambda: ctx.anchor_begin(sizes, changed(tables[0], 7, 99), *tables[1:], tgt, WINDOW), word="scaffold 7 ")
            refused(lambda: ctx.anchor_begin(sizes, tables[0], changed(tables[1], 4, tables[1][17]), *tables[2:], tgt, WINDOW), word="overlap")
        # no candidate: every scaffold placed, or no scaffold with a target
        everything = lref.layout([[(s, "+") for s in range(40)]], sizes, 0, drop_unplaced=True)
        refused(lambda: ctx.anchor_begin(sizes, *everything, None, WINDOW), word="no candidate")
        refused(lambda: ctx.anchor_begin(sizes, *tables, np.full(40, -1, np.int32), WINDOW), word="no candidate")
        refused(lambda: ctx.anchor_begin(sizes, *tables, changed(target, a_candidate, 3), WINDOW), word="scaffold %d " % a_candidate)
        refused(lambda: ctx.anchor_begin(sizes, *tables, changed(target, a_candidate, -2), WINDOW), word="scaffold %d " % a_candidate)
        refused(lambda: ctx.anchor_begin(sizes, *tables, changed(target, 3, 0), WINDOW), word="scaffold 3 ")       # a placed scaffold
        empty = changed(sizes, a_candidate, 0)
        refused(lambda: ctx.anchor_begin(empty, *lref.layout(CHROMS, empty, 100, drop_unplaced=True), target, WINDOW),
                word="scaffold %d " % a_candidate)                                                               # a target on an empty one
        hollow = changed(sizes, [s for s, _o in CHROMS[2]], 0)                                                    # Chr_3 without a base: S_q = 0
        refused(lambda: ctx.anchor_begin(hollow, *lref.layout(CHROMS, hollow, 100, drop_unplaced=True), target, WINDOW), word="sequence")
        # 2^14 + 1 candidates against 2^13 sequences: one block past 2^27 counters - sizes only, nothing that large is allocated
        n_seq, many = 2 ** 13, 2 ** 13 + 2 ** 14 + 1
        wide = lref.layout([[(q, "+")] for q in range(n_seq)], np.ones(many, np.int64), 0, drop_unplaced=True)
        refused(lambda: ctx.anchor_begin(np.ones(many, np.int64), *wide, None, 1), code=EUNSUPPORTED, word="counters")
        S, many = 2 ** 12, 2 ** 12 + 2 ** 13 + 1
        deep = lref.layout([[(s, "+") for s in range(S)]], np.ones(many, np.int64), 0, drop_unplaced=True)
        refused(lambda: ctx.anchor_begin(np.ones(many, np.int64), *deep, np.where(np.arange(many) < S, -1, 0).astype(np.int32), 1),
                code=EUNSUPPORTED, word="counters")
        refused(lambda: ctx.anchor_finish(), word="without")                 # none of them opened a build
        first = ctx.anchor_begin(sizes, *tables, target, WINDOW)
        assert first.tolist() == want[0].tolist()
        ctx.anchor_add_pairs(*_first(pairs, 1000))
        refused(lambda: ctx.anchor_begin(sizes, *tables, target, 0))          # a refused begin leaves the open build open
        refused(lambda: ctx.anchor_add_pairs(changed(sa, 200, len(sizes)), pa, sb, pb), word="pair 200 ")
        refused(lambda: ctx.anchor_add_pairs(sa, pa, sb, changed(pb, 100, sizes[sb[100]] + 1)), word="pair 100 ")
        refused(lambda: ctx.anchor_add_pairs(sa, changed(pa, 4000, 0), sb, pb), word="pair 4000 ")
        untouched(ctx)
        ctx.anchor_add_pairs(*tuple(a[1000:] for a in pairs))                 # the build is still open, and right
        _same((first,) + ctx.anchor_finish(), want)
        refused(lambda: ctx.anchor_finish(), word="without")                 # ... and closed now
        # a begin gives an open anchor build up
        ctx.anchor_begin(sizes, *tables, target, 1)
        ctx.anchor_add_pairs(*pairs)
        first = ctx.anchor_begin(sizes, *tables, None, WINDOW)
        ctx.anchor_add_pairs(*pairs)
        _same((first,) + ctx.anchor_finish(), want_seq)
        untouched(ctx)
        # the ends, span and map builds that were open all the while take the rest of their pairs and are what they would have been
        ctx.ends_add_pairs(*tuple(a[half:] for a in pairs))
        got_T, got_counters = ctx.ends_finish()
        assert got_T.tobytes() == ends_T.tobytes() and got_counters.tolist() == ends_counters.tolist()
        ctx.span_add_pairs(*tuple(a[half:] for a in pairs))
        picks, counters, depth = ctx.span_finish(3, span_recs)
        assert depth.tobytes() == span_D.tobytes() and counters.tolist() == span_counters.tolist() and picks.tolist() == span_picks.tolist()
        ctx.map_add_pairs(*tuple(a[half:] for a in pairs))
        assert ctx.map_finish() == n and ctx.contacts_host().tobytes() == map_want.tobytes()
    ctx = _lib.Context(0)                                                     # a context destroyed between begin and finish
    ctx.anchor_begin(sizes, *tables, target, WINDOW)
    ctx.anchor_add_pairs(*pairs)
    ctx.close()


# ---- the one-pass driver -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _odd_file():
    names, sizes = _scaffolds()
    data = bref.odd_file_bytes(names, sizes, 3000, seed=23)                   # CR LF lines, twelve columns, lines that are skipped
    pairs, stats, _after = bref.parse_text(data, names, sizes)
    more = ref.pair_file_bytes(names, _pool())
    pairs = tuple(np.concatenate([a, b]) for a, b in zip(pairs, _pool()))
    assert b"\r\n" in data and stats[2] > 50 and stats[3] > 50
    return data + b"\n" + more, (stats[0] + COUNTS[-1], stats[1] + COUNTS[-1], stats[2], stats[3]), pairs


def _write(tmp_path, data):
    path = str(tmp_path / "pairs.allValidPairs")
    with open(path, "wb") as fh:
        fh.write(data)
    return path


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("chunk", ["1000", None])
def test_anchor_file_equals_the_array_calls(chunk, mode, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, stats, pairs = _odd_file()
    tables, target = _tables(), _target(mode)
    want = _want(pairs, sizes, tables, target, WINDOW)
    path = _write(tmp_path, data)
    _set_form(monkeypatch, form)
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held + held.T)
        got_stats, first, T, counters = _lib.anchor_file(path, names, sizes, *tables, target, WINDOW, ctx, threads=2)
        assert got_stats[:4] == stats and got_stats[4] == (-(-stats[1] // 1000) if chunk else 1) and stats[1] >= 3 * 1000
        _same((first, T, counters), want)
        assert int(counters.sum()) == stats[1]
        assert ctx.n == 4 and ctx.contacts_host().tobytes() == (held + held.T).tobytes()
        with pytest.raises(_lib.HicmiError):
            ctx.anchor_finish()                                               # no build is left open
        _same(_run(sizes, tables, target, WINDOW, [pairs], ctx), want)        # the array calls on the file's pairs


def test_anchor_file_error_writes_no_output(tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, _stats, pairs = _odd_file()
    tables, target = _tables(), _target("rank")
    want = _want(pairs, sizes, tables, target, WINDOW)
    _set_form(monkeypatch, "default")
    monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", "1000")
    lib = _lib.load()
    blob, off = _lib._name_blob(names)
    size, seq, loff, rev, seq_size = _lib._lift_tables(sizes, *tables)

    def call(ctx, path, window=WINDOW, tgt=target, tables5=(size, seq, loff, rev, seq_size)):
        outs = [np.full(5, -7, np.int64), np.full(len(want[1]), 77, np.uint64), np.full(6, 77, np.uint64), np.full(len(size), -7, np.int64)]
        n_table = ctypes.c_int64(-7)
        sz, sq, lo, rv, ss = tables5
        rc = lib.hicmi_anchor_file(os.fsencode(path), blob, _lib._ptr(off), len(names), _lib._ptr(sz), _lib._ptr(sq), _lib._ptr(lo),
                                   _lib._ptr(rv), _lib._ptr(ss), len(ss), _lib._ptr(tgt), window, ctx._h, 2, _lib._ptr(outs[0]),
                                   _lib._ptr(outs[1]), _lib._ptr(outs[2]), _lib._ptr(outs[3]), ctypes.byref(n_table))
        return rc, outs, n_table.value, lib.hicmi_last_error().decode()

    def unwritten(outs, n_table):
        return n_table == -7 and all((o == -7).all() for o in (outs[0], outs[3])) and all((o == 77).all() for o in outs[1:3])

    assert data.endswith(b"\n")
    bad = _write(tmp_path, data + b"read\tscaffold_4\t12x\t+\tscaffold_4\t5\n")
    with _lib.Context(0) as ctx:
        rc, outs, n_table, message = call(ctx, bad)
        assert rc == EINVAL and message.endswith("at byte %d" % len(data)) and unwritten(outs, n_table)
        with pytest.raises(_lib.HicmiError):
            ctx.anchor_finish()                                               # no build is left open
        good = _write(tmp_path, data)
        a_candidate = int(np.flatnonzero(target >= 0)[0])
        bad_target = np.array(target)
        bad_target[a_candidate] = 3
        for kwargs in ({"window": 0}, {"tgt": bad_target}, {"tgt": np.full(40, -1, np.int32)},
                       {"tables5": (size, np.where(seq < 0, 99, seq).astype(np.int32), loff, rev, seq_size)}):
            rc, outs, n_table, message = call(ctx, good, **kwargs)
            assert rc == EINVAL and unwritten(outs, n_table), message
        rc, outs, n_table, message = call(ctx, str(tmp_path / "missing"))
        assert rc == EINVAL and "cannot open" in message and unwritten(outs, n_table)
        with pytest.raises(_lib.HicmiError):
            ctx.anchor_finish()
        rc, outs, n_table, message = call(ctx, good)
        assert rc == 0 and n_table == len(want[1])
        _same((outs[3], outs[1], outs[2]), want)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip_on_the_planted_scaffolds(tmp_path, monkeypatch, capsys):
    """device == reference == plant: the eight scaffolds taken out of the order file return to their chromosome, gap and
    orientation, seven in the first run and the deferred one in a second run on the -placed file."""
    from hic_genome_assembler_amd import _lib, placeUnplaced
    import test_anchor_cpu as cpu
    _set_form(monkeypatch, "default")
    P, (result, winners), chroms, (result2, winners2) = cpu.planted_rounds()
    order_text = lref.order_file_text(P["chroms"], P["names"])
    cfg, order, save, _paths = cpu._case_files(tmp_path, P["names"], P["sizes"], order_text, P["pairs"])
    placed, full = str(tmp_path / "placed.txt"), str(tmp_path / "full")
    args = ["-window", "%d" % ref.PLANTED_WINDOW, "-threads", "3"]
    _stats, verdicts, inserted = placeUnplaced.main(["-config", cfg, "-order", order, "-placed", placed, "-full", full] + args)
    assert "UNPLACED: 8 unplaced scaffold(s), 8 with a chromosome, 7 inserted, 1 deferred" in capsys.readouterr().out
    report = cpu._read(os.path.join(save, "unplacedSupport.txt"))
    want, want_winners, _result = cpu.expected_report(P["names"], P["sizes"], P["chroms"], P["pairs"], ref.PLANTED_WINDOW, ref.PLANTED_REACH,
                                                      ref.PLANTED_MIN_PAIRS, ref.PLANTED_MIN_RATIO, 0)
    assert report == want and want_winners == winners
    truth = ref.planted_truth(P)
    assert inserted == {P["names"][c]: truth[c] for c in winners.values()} and len(inserted) == 7
    assert {s: v for s, v in verdicts.items()} == {c: r["verdict"] for c, r in result.items()}
    assert cpu._read(placed) == ref.placed_text(order_text, P["names"], P["sizes"], P["chroms"], result, winners)
    assert cpu._read(placed) == lref.order_file_text(chroms, P["names"])
    # a context of the caller's, driven through the array calls, writes the same bytes
    out2 = str(tmp_path / "again.txt")
    with _lib.Context(0) as ctx:
        placeUnplaced.main(["-config", cfg, "-order", order, "-out", out2] + args, context=ctx)
    assert cpu._read(out2) == report
    # the second run, on the placed file: the deferred scaffold goes in next to the winner of its gap
    out3, placed3 = str(tmp_path / "third.txt"), str(tmp_path / "placed3.txt")
    _stats, verdicts3, inserted3 = placeUnplaced.main(["-config", cfg, "-order", placed, "-out", out3, "-placed", placed3] + args)
    assert verdicts3 == {29: "placed"} and inserted3 == {P["names"][29]: ref.planted_truth(P, chroms)[29]}
    assert cpu._read(out3) == cpu.expected_report(P["names"], P["sizes"], chroms, P["pairs"], ref.PLANTED_WINDOW, ref.PLANTED_REACH,
                                                  ref.PLANTED_MIN_PAIRS, ref.PLANTED_MIN_RATIO, 0)[0]
    assert cpu._read(placed3) == lref.order_file_text(P["true_chroms"], P["names"])
