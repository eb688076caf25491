"""End support on the device (hicmi_ends_begin / _add_pairs / _finish / _file) against
tests/ends_reference.py, for HICMI_ENDS_PLAIN unset, =1 and =0.  Ranks, table and counters are integers, so every
comparison is exact: there are no tolerances."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import buildmap_reference as bref
import ends_reference as ref
import liftmap_reference as lref
import span_reference as sref

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -5
# Both count forms give the same bits by design: these tests hold each to the reference but cannot tell which kernel ran; that
# the switch is read per call is checked from the source in tests/test_ends_cpu.py.
FORMS = {"default": {}, "plain": {"HICMI_ENDS_PLAIN": "1"}, "combine": {"HICMI_ENDS_PLAIN": "0"}}
FORM_NAMES = ["default", "plain", "combine"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    with open(os.path.join(ROOT, "hic_genome_assembler_amd", "csrc", "hicmi_internal.h")) as fh:
        text = fh.read()
    value = re.search(r"static constexpr int %s = ([^;]+);" % name, text).group(1)
    return 1 << _constant(value.split("<<")[1].strip()) if "<<" in value else int(value)


SLICE, SLOT_BITS, SLOTS, PROBES = (_constant(k) for k in ("ENDS_SLICE", "ENDS_SLOT_BITS", "ENDS_SLOTS", "ENDS_PROBES"))
COUNTS = [1, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 5000]
WINDOW, REACH = 500, 2
# three chromosomes of mixed orientations on the 40 odd scaffolds (sizes 1, 999, 1000, 1001, 3007 and three of 70,000)
CHROMS = [[(3, "+"), (0, "-"), (4, "-"), (17, "+"), (1, "-"), (2, "+"), (7, "-")],
          [(38, "-"), (5, "-"), (6, "+"), (9, "-"), (8, "+"), (11, "+"), (12, "-"), (13, "-")],
          [(20, "-"), (21, "+"), (22, "-"), (24, "+"), (23, "-")]]
ONE_CHROM = [[(s, "+-"[s % 3 == 0]) for s in (list(range(20, 40)) + list(range(20)))]]


def _set_form(monkeypatch, form):
    for key in ("HICMI_ENDS_PLAIN", "HICMI_SPANS_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS", "HICMI_BUILDMAP_PLAIN", "HICMI_LIFTMAP_PLAIN"):
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
def _one_chromosome():
    _names, sizes = _scaffolds()
    return _frozen(*lref.layout(ONE_CHROM, sizes, 100))


@functools.lru_cache(maxsize=None)
def _pool():
    """5,000 pairs: most of them between two scaffolds of one chromosome, the ends of the long scaffolds favoured, some on
    one scaffold, some anywhere."""
    _names, sizes = _scaffolds()
    rng = np.random.default_rng(5)
    n = COUNTS[-1]
    members = [np.array([s for s, _o in ch]) for ch in CHROMS]
    ch = rng.integers(0, 3, n)
    sa = np.array([rng.choice(members[c]) for c in ch])
    sb = np.array([rng.choice(members[c]) for c in ch])

    def positions(s):
        L = sizes[s]
        p = 1 + np.floor(rng.random(n) * L).astype(np.int64)
        edge = rng.integers(0, 6, n)                                  # the first or the last 600 bases, where there are that many
        near = np.minimum(rng.integers(1, 601, n), L)
        near[edge >= 4] = 1                                           # ... and the very first and last base
        return np.where(edge % 2 == 0, near, L + 1 - near) * (edge != 2) * (edge != 3) + p * ((edge == 2) | (edge == 3))

    pa, pb = positions(sa), positions(sb)
    kind = rng.integers(0, 10, n)
    same = kind <= 1
    sb[same] = sa[same]
    pb[same] = np.clip(pa[same] + rng.integers(-700, 700, same.sum()), 1, sizes[sa[same]])
    anywhere = kind == 9
    sb[anywhere] = rng.integers(0, 40, anywhere.sum())
    pb[anywhere] = 1 + np.floor(rng.random(anywhere.sum()) * sizes[sb[anywhere]]).astype(np.int64)
    return _frozen(sa.astype(np.int32), pa, sb.astype(np.int32), pb)


def _first(pairs, n):
    return tuple(a[:n] for a in pairs)


def _want(pairs, sizes, tables, window, reach):
    T, counters = ref.table(pairs, sizes, tables, window, reach)
    rank, seq_first, n = ref.number_ranks(sizes, tables)
    assert T.shape == (n, reach, 4) and not ref.outside(T, seq_first).any()
    assert int(counters.sum()) == len(pairs[0]) and int(T.sum()) == int(counters[ref.LINKED])
    return rank, T, counters, seq_first


def _run(sizes, tables, window, reach, parts, ctx=None):
    from hic_genome_assembler_amd import _lib
    if ctx is None:
        with _lib.Context(0) as own:
            return _run(sizes, tables, window, reach, parts, own)
    rank = ctx.ends_begin(sizes, *tables, window, reach)
    for p in parts:
        ctx.ends_add_pairs(*p)
    return (rank,) + ctx.ends_finish()


def _same(got, want):
    rank, T, counters, seq_first = want
    assert got[0].dtype == np.int32 and got[0].tolist() == rank.tolist()
    assert got[1].dtype == np.uint64 and got[1].shape == T.shape and got[1].tobytes() == T.tobytes()
    assert not ref.outside(got[1], seq_first).any()                         # entries that leave a sequence are 0
    assert got[2].dtype == np.uint64 and got[2].tolist() == counters.tolist()


# ---- pair counts, windows, reaches, kinds of pairs ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_pool(n, gap, drop, window, reach):
    _names, sizes = _scaffolds()
    return _want(_first(_pool(), n), sizes, _tables(gap, drop), window, reach)


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("n", COUNTS)
def test_pair_counts_at_the_wave_workgroup_and_slice_edges(n, form, monkeypatch):
    _names, sizes = _scaffolds()
    want = _want_pool(n, 100, False, WINDOW, REACH)
    _set_form(monkeypatch, form)
    _same(_run(sizes, _tables(100, False), WINDOW, REACH, [_first(_pool(), n)]), want)


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("drop", [False, True])
def test_windows_reaches_and_the_six_counters(drop, form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    assert max(len(ch) for ch in CHROMS) < 64                               # a reach of 64 is longer than every chromosome
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        for gap in (0, 100):
            for window in (1, 500, 10 ** 9):
                for reach in (1, 2, 64):
                    want = _want_pool(COUNTS[-1], gap, drop, window, reach)
                    linked, middle, same, far, trans, unlifted = want[2].tolist()
                    assert linked > 50 and same > 500 and trans > 100 and (unlifted > 100) == drop
                    assert (far > 300) == (reach < 64) and (middle > 100) == (window < 10 ** 9)
                    _same(_run(sizes, _tables(gap, drop), window, reach, [_pool()], ctx), want)


# ---- the table in LDS --------------------------------------------------------------------------------------------------------------------
def _replay_spills(index):
    """The pairs of one slice that find no room in the table of the combining kernel, taken in index order: the hash and
    the probe rule of ends_add_lds in NumPy integers."""
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
    """All 40 scaffolds in one chromosome at reach 64 and a huge window, the scaffolds of every pair drawn uniformly: nearly
    every pair is linked, and the first slice alone holds more distinct counters than the table has slots."""
    _names, sizes = _scaffolds()
    rng = np.random.default_rng(17)
    n = 2 * SLICE + 300
    sa, sb = rng.integers(0, 40, n), rng.integers(0, 40, n)
    pa = 1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64)
    return _frozen(sa.astype(np.int32), pa, sb.astype(np.int32), pb)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_a_slice_with_more_counters_than_the_probes_can_place(form, monkeypatch):
    _names, sizes = _scaffolds()
    tables, pairs = _one_chromosome(), _crowded()
    kind, index = ref.classify(_first(pairs, SLICE), sizes, tables, 10 ** 9, 64)
    first_slice = index[kind == ref.LINKED]
    # whatever order the lanes arrive in, a table of SLOTS slots cannot hold more distinct counters than that; taken in
    # index order, the replay of the probe rule says how many pairs it turns away
    assert len(np.unique(first_slice)) > SLOTS and _replay_spills(first_slice) >= 1
    want = _want(pairs, sizes, tables, 10 ** 9, 64)
    assert want[2][ref.LINKED] > 2 * SLICE and want[1].max() < 20
    _set_form(monkeypatch, form)
    _same(_run(sizes, tables, 10 ** 9, 64, [pairs]), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_slices_whose_pairs_all_hit_one_counter(form, monkeypatch):
    _names, sizes = _scaffolds()
    tables = _tables(100, False)
    n = 3 * SLICE + 5
    # base 5 of scaffold 4, the first of its chromosome, and base 69,900 of scaffold 18, three places on: LEFT and RIGHT
    pairs = tuple(np.full(n, v, dtype=t) for v, t in ((3, np.int32), (5, np.int64), (17, np.int32), (69900, np.int64)))
    want = _want(pairs, sizes, tables, WINDOW, 3)
    assert want[2].tolist() == [n, 0, 0, 0, 0, 0] and np.flatnonzero(want[1].reshape(-1)).tolist() == [(0 * 3 + 2) * 4 + ref.LR]
    _set_form(monkeypatch, form)
    _same(_run(sizes, tables, WINDOW, 3, [pairs]), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_any_chunking_and_any_order_give_the_same_bits(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = _scaffolds()
    want = _want_pool(COUNTS[-1], 100, True, WINDOW, REACH)
    pairs = _pool()
    n = COUNTS[-1]
    order = np.random.default_rng(9).permutation(n)
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        for cuts in ([0, n], [0, 100, n], [0, 1, 257, 258, 2500, 2500, SLICE + 2500, n]):
            assert len(cuts) - 1 in (1, 2, 7)
            parts = [tuple(a[lo:hi] for a in pairs) for lo, hi in zip(cuts, cuts[1:])]
            _same(_run(sizes, _tables(100, True), WINDOW, REACH, parts, ctx), want)
        _same(_run(sizes, _tables(100, True), WINDOW, REACH, [tuple(a[order] for a in pairs)], ctx), want)
        swapped = (pairs[2], pairs[3], pairs[0], pairs[1])                    # the mates of every pair exchanged
        _same(_run(sizes, _tables(100, True), WINDOW, REACH, [swapped], ctx), want)


# ---- 64-bit positions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
def test_scaffolds_of_2_to_the_33(form, monkeypatch):
    L = 2 ** 33
    sizes = np.array([L, L + 1, L], dtype=np.int64)
    tables = lref.layout([[(0, "+"), (1, "-"), (2, "+")]], sizes, 100)
    rng = np.random.default_rng(3)
    n = 3000
    _set_form(monkeypatch, form)
    for window in (2 ** 20, 2 ** 32 + 1, 2 ** 62):
        edge = np.array([1, 2, window, window + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, L // 2, L // 2 + 1, L - window, L - window + 1, L - 1, L])
        edge = edge[(edge >= 1) & (edge <= L)]
        sa, sb = rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32)
        pa = np.where(rng.random(n) < 0.5, rng.choice(edge, n), rng.integers(1, L + 1, n))
        pb = np.where(rng.random(n) < 0.5, rng.choice(edge, n), rng.integers(1, L + 1, n))
        want = _want((sa, pa, sb, pb), sizes, tables, window, 2)
        assert want[2][ref.LINKED] > 50 and want[2][ref.SAME] > 500 and (want[2][ref.MIDDLE] > 300) == (window < L // 2)
        _same(_run(sizes, tables, window, 2, [(sa, pa, sb, pb)]), want)


# ---- misuse --------------------------------------------------------------------------------------------------------------------------------------
def test_misuse_leaves_the_matrix_an_open_map_build_and_an_open_span_build_as_they_were(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    _names, sizes = _scaffolds()
    tables = _tables(100, True)
    pairs = _pool()
    n = COUNTS[-1]
    half = n // 2
    want = _want_pool(n, 100, True, WINDOW, REACH)
    map_want = bref.build(pairs, sizes, bref.R)
    span_recs = [(0, 10, 0, int(sref.number_cells(sizes, tables, 500)[1][1]))]
    span_D, span_counters, _marks = sref.depth(pairs, sizes, tables, 500)
    span_picks = sref.picks(span_D, 3, span_recs)
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
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held)
        ctx.map_begin(sizes, bref.R)                                          # a map build and a span build stay open through all of this
        ctx.map_add_pairs(*_first(pairs, half))
        ctx.span_begin(sizes, *tables, 500)
        ctx.span_add_pairs(*_first(pairs, half))
        refused(lambda: ctx.ends_finish(), word="without")
        refused(lambda: ctx.ends_add_pairs(*pairs), word="without")
        refused(lambda: ctx.ends_begin(sizes, *tables, 0, REACH), word="window")
        refused(lambda: ctx.ends_begin(sizes, *tables, WINDOW, 0), word="reach")
        refused(lambda: ctx.ends_begin(sizes, *tables, WINDOW, 65), word="reach")
        refused(lambda: ctx.ends_begin(sizes, changed(tables[0], 7, 99), *tables[1:], WINDOW, REACH), word="scaffold 7 ")
        refused(lambda: ctx.ends_begin(sizes, tables[0], changed(tables[1], 4, tables[1][17]), *tables[2:], WINDOW, REACH), word="overlap")
        refused(lambda: ctx.ends_begin(sizes, np.full(40, -1, np.int32), *tables[1:], WINDOW, REACH), word="no scaffold")
        # 2^19 + 1 placed scaffolds at reach 64: one entry past 2^27 counters; 2^19 at reach 64 would fit
        many = 2 ** 19 + 1
        refused(lambda: ctx.ends_begin(np.ones(many, np.int64), np.zeros(many, np.int32), np.arange(many), np.zeros(many, np.uint8), [many], 1, 64),
                code=EUNSUPPORTED, word="counters")
        refused(lambda: ctx.ends_finish(), word="without")                   # none of them opened a build
        rank = ctx.ends_begin(sizes, *tables, WINDOW, REACH)
        assert rank.tolist() == want[0].tolist()
        ctx.ends_add_pairs(*_first(pairs, 1000))
        refused(lambda: ctx.ends_begin(sizes, *tables, 0, REACH))             # a refused begin leaves the open build open
        refused(lambda: ctx.ends_add_pairs(changed(sa, 200, len(sizes)), pa, sb, pb), word="pair 200 ")
        refused(lambda: ctx.ends_add_pairs(sa, pa, sb, changed(pb, 100, sizes[sb[100]] + 1)), word="pair 100 ")
        refused(lambda: ctx.ends_add_pairs(sa, changed(pa, 4000, 0), sb, pb), word="pair 4000 ")
        untouched(ctx)
        ctx.ends_add_pairs(*tuple(a[1000:] for a in pairs))                   # the build is still open, and right
        _same((rank,) + ctx.ends_finish(), want)
        refused(lambda: ctx.ends_finish(), word="without")                   # ... and closed now
        # a begin gives an open ends build up
        ctx.ends_begin(sizes, *tables, 1, 64)
        ctx.ends_add_pairs(*pairs)
        ctx.ends_begin(sizes, *tables, WINDOW, REACH)
        ctx.ends_add_pairs(*pairs)
        _same((rank,) + ctx.ends_finish(), want)
        untouched(ctx)
        # the span build and the map build that were open all the while take the rest of their pairs and are what they would have been
        ctx.span_add_pairs(*tuple(a[half:] for a in pairs))
        picks, counters, depth = ctx.span_finish(3, span_recs)
        assert depth.tobytes() == span_D.tobytes() and counters.tolist() == span_counters.tolist() and picks.tolist() == span_picks.tolist()
        ctx.map_add_pairs(*tuple(a[half:] for a in pairs))
        assert ctx.map_finish() == n and ctx.contacts_host().tobytes() == map_want.tobytes()
    ctx = _lib.Context(0)                                                     # a context destroyed between begin and finish
    ctx.ends_begin(sizes, *tables, WINDOW, REACH)
    ctx.ends_add_pairs(*pairs)
    ctx.close()


# ---- the one-pass driver -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _odd_file():
    names, sizes = _scaffolds()
    data = bref.odd_file_bytes(names, sizes, 5000, seed=23)
    pairs, stats, _after = bref.parse_text(data, names, sizes)
    tables = _tables(100, True)
    # the file's scaffolds are drawn at random: give the table something to count with pairs inside the chromosomes
    more = ref.pair_file_bytes(names, _pool())
    pairs = tuple(np.concatenate([a, b]) for a, b in zip(pairs, _pool()))
    return data + b"\n" + more, (stats[0] + COUNTS[-1], stats[1] + COUNTS[-1], stats[2], stats[3]), tables, \
        _want(pairs, sizes, tables, WINDOW, REACH), pairs


def _write(tmp_path, data):
    path = str(tmp_path / "pairs.allValidPairs")
    with open(path, "wb") as fh:
        fh.write(data)
    return path


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("threads", [1, 0])
@pytest.mark.parametrize("chunk", ["1000", None])
def test_ends_file_equals_the_array_calls(chunk, threads, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, stats, tables, want, pairs = _odd_file()
    path = _write(tmp_path, data)
    _set_form(monkeypatch, form)
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held + held.T)
        got_stats, rank, T, counters = _lib.ends_file(path, names, sizes, *tables, WINDOW, REACH, ctx, threads=threads)
        assert got_stats[:4] == stats and got_stats[4] == (-(-stats[1] // 1000) if chunk else 1) and stats[1] > 4 * 1000
        _same((rank, T, counters), want)
        assert int(counters[ref.UNLIFTED]) > 500 and int(counters.sum()) == stats[1]
        assert ctx.n == 4 and ctx.contacts_host().tobytes() == (held + held.T).tobytes()
        with pytest.raises(_lib.HicmiError):
            ctx.ends_finish()                                                 # no build is left open
        _same(_run(sizes, tables, WINDOW, REACH, [pairs], ctx), want)         # the array calls on the file's pairs


@pytest.mark.parametrize("chunk", ["1000", None])
def test_ends_file_error_writes_no_output(chunk, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, _stats, tables, want, _pairs = _odd_file()
    _set_form(monkeypatch, "default")
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    lib = _lib.load()
    blob, off = _lib._name_blob(names)
    size, seq, loff, rev, seq_size = _lib._lift_tables(sizes, *tables)
    shape = want[1].shape

    def call(ctx, path, window=WINDOW, reach=REACH, tables5=(size, seq, loff, rev, seq_size), n_names=len(names)):
        outs = [np.full(5, -7, np.int64), np.full(shape, 77, np.uint64), np.full(6, 77, np.uint64), np.full(len(size), -7, np.int32)]
        n_placed = ctypes.c_int64(-7)
        sz, sq, lo, rv, ss = tables5
        rc = lib.hicmi_ends_file(os.fsencode(path), blob, _lib._ptr(off), n_names, _lib._ptr(sz), _lib._ptr(sq), _lib._ptr(lo),
                                 _lib._ptr(rv), _lib._ptr(ss), len(ss), window, reach, ctx._h, 2, _lib._ptr(outs[0]), _lib._ptr(outs[1]),
                                 _lib._ptr(outs[2]), _lib._ptr(outs[3]), ctypes.byref(n_placed))
        return rc, outs, n_placed.value, lib.hicmi_last_error().decode()

    def unwritten(outs, n_placed):
        return n_placed == -7 and all((o == -7).all() for o in (outs[0], outs[3])) and all((o == 77).all() for o in outs[1:3])

    assert data.endswith(b"\n")
    bad = _write(tmp_path, data + b"read\tscaffold_4\t12x\t+\tscaffold_4\t5\n")
    with _lib.Context(0) as ctx:
        rc, outs, n_placed, message = call(ctx, bad)
        assert rc == EINVAL and message.endswith("at byte %d" % len(data)) and unwritten(outs, n_placed)
        with pytest.raises(_lib.HicmiError):
            ctx.ends_finish()                                                 # no build is left open
        good = _write(tmp_path, data)
        for kwargs in ({"window": 0}, {"reach": 0}, {"reach": 65}, {"tables5": (size, np.full(40, -1, np.int32), loff, rev, seq_size)}):
            rc, outs, n_placed, message = call(ctx, good, **kwargs)
            assert rc == EINVAL and unwritten(outs, n_placed), message
        # a table past the limit: 2^25 / 48 + 1 scaffold sizes at reach 48 (the names beyond the 40 are never looked at)
        many = 2 ** 25 // 48 + 1
        huge = (np.ones(many, np.int64), np.zeros(many, np.int32), np.arange(many, dtype=np.int64), np.zeros(many, np.uint8), np.array([many], np.int64))
        big_blob, big_off = _lib._name_blob(["s%d" % k for k in range(many)])
        outs = [np.full(5, -7, np.int64), np.full(4, 77, np.uint64), np.full(6, 77, np.uint64), np.full(many, -7, np.int32)]
        n_placed = ctypes.c_int64(-7)
        rc = lib.hicmi_ends_file(os.fsencode(good), big_blob, _lib._ptr(big_off), many, *(_lib._ptr(x) for x in huge[:4]), _lib._ptr(huge[4]), 1, 1,
                                 48, ctx._h, 2, _lib._ptr(outs[0]), _lib._ptr(outs[1]), _lib._ptr(outs[2]), _lib._ptr(outs[3]), ctypes.byref(n_placed))
        assert rc == EUNSUPPORTED and unwritten(outs, n_placed.value)
        rc, outs, n_placed, message = call(ctx, str(tmp_path / "missing"))
        assert rc == EINVAL and "cannot open" in message and unwritten(outs, n_placed)
        with pytest.raises(_lib.HicmiError):
            ctx.ends_finish()
        rc, outs, n_placed, message = call(ctx, good)
        assert rc == 0 and n_placed == shape[0]
        _same((outs[3], outs[1], outs[2]), want)


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip_on_the_planted_flips(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import _lib, supportEnds
    import test_ends_cpu as cpu
    _set_form(monkeypatch, "default")
    cfg, order, save, _paths = cpu._planted_files(tmp_path)
    flipped, full = str(tmp_path / "flipped.txt"), str(tmp_path / "full")
    supportEnds.main(["-config", cfg, "-order", order, "-window", "5000", "-flipped", flipped, "-full", full, "-threads", "3"])
    assert "ENDS: 10 scaffold(s) to flip, 0 open" in capsys.readouterr().out
    report = cpu._read(os.path.join(save, "endSupport.txt"))
    cpu.check_planted_outputs(report, cpu._read(flipped), cpu._read(os.path.join(full, "ends.links.tsv")))
    # a context of the caller's, driven through the array calls, writes the same bytes
    out2 = str(tmp_path / "again.txt")
    with _lib.Context(0) as ctx:
        supportEnds.main(["-config", cfg, "-order", order, "-window", "5000", "-out", out2], context=ctx)
    assert cpu._read(out2) == report
    # on the flipped order file nothing is left to flip
    out3 = str(tmp_path / "third.txt")
    supportEnds.main(["-config", cfg, "-order", flipped, "-window", "5000", "-out", out3])
    third = cpu._read(out3)
    assert "\tflip\n" not in third and third.count("\tsupported\n") == 40 and third.count("\theld\n") == 37
