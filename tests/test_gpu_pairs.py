"""The resident pair store on the device (hicmi_pairs_*, hicmi_ends_resident, hicmi_anchor_resident) against
tests/pairs_reference.py and the file calls, for HICMI_PAIRS_PLAIN unset and =1.  The stable form's store is compared as it
is, the plain form's by sorted rows; tables and counters are integers, so every comparison is exact."""
import ctypes
import functools
import os

import numpy as np
import pytest

import anchor_reference as aref
import buildmap_reference as bref
import ends_reference as eref
import liftmap_reference as lref
import pairs_reference as ref
import span_reference as sref
import test_gpu_anchor as ga
import test_gpu_ends as ge

pytestmark = pytest.mark.gpu
EINVAL = -1
FORMS = {"default": {}, "plain": {"HICMI_PAIRS_PLAIN": "1"}}
FORM_NAMES = ["default", "plain"]
SLICE = ge._constant("PAIRS_SLICE")
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 17]
PATTERNS = ["all", "none", "alternating", "first", "last"]
WINDOW, REACH = ge.WINDOW, ge.REACH


def _set_form(monkeypatch, form):
    for key in ("HICMI_PAIRS_PLAIN", "HICMI_PAIRS_FIRST_PAIRS", "HICMI_ENDS_PLAIN", "HICMI_ANCHOR_PLAIN", "HICMI_SPANS_PLAIN",
                "HICMI_BUILDMAP_CHUNK_PAIRS", "HICMI_BUILDMAP_PLAIN", "HICMI_LIFTMAP_PLAIN"):
        monkeypatch.delenv(key, raising=False)
    for key, value in FORMS[form].items():
        monkeypatch.setenv(key, value)


def _patterned(n, pattern, seed=3):
    """n pairs on the 40 odd scaffolds that have two bases or more, kept as the pattern says."""
    _names, sizes = ge._scaffolds()
    rng = np.random.default_rng(seed + n)
    have = np.flatnonzero(sizes > 1)
    sa = rng.choice(have, n)
    other = rng.choice(have, n)
    other = np.where(other == sa, have[(np.searchsorted(have, sa) + 1) % len(have)], other)
    k = np.arange(n)
    kept = {"all": k >= 0, "none": k < 0, "alternating": k % 2 == 0, "first": k == 0, "last": k == n - 1}[pattern]
    sb = np.where(kept, other, sa)
    pa = 1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64)
    pairs = (sa.astype(np.int32), pa, sb.astype(np.int32), pb)
    assert ref.mask(pairs).tolist() == kept.tolist()
    return pairs


def _same_store(ctx, pairs, n_scaf, form):
    """The store and intra[] of ``ctx`` against the NumPy mask and bincount of ``pairs``."""
    want, counts = ref.keep(pairs), ref.intra(pairs, n_scaf)
    n_kept, n_intra, intra = ctx.pairs_info()
    assert n_kept == len(want[0]) and n_intra == int(counts.sum()) and intra.dtype == np.uint64 and intra.tolist() == counts.tolist()
    got = ctx.pairs_fetch()
    assert [a.dtype for a in got] == [np.int32, np.int64, np.int32, np.int64] and all(len(a) == n_kept for a in got)
    if form == "plain":
        assert ref.sorted_rows(got).tobytes() == ref.sorted_rows(want).tobytes()
    else:
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    return got


# ---- sizes, patterns, chunking -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_sizes_at_the_wave_workgroup_and_slice_edges(pattern, form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = ge._scaffolds()
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        for n in COUNTS:
            pairs = _patterned(n, pattern)
            ctx.pairs_begin(sizes)
            ctx.pairs_add(*pairs)
            _same_store(ctx, pairs, len(sizes), form)
            ctx.pairs_drop()


@pytest.mark.parametrize("form", FORM_NAMES)
def test_chunks_of_1_7_a_slice_and_the_rest_give_the_store_of_one_call(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = ge._scaffolds()
    pairs = ge._pool()                                                          # a fifth of its pairs lie on one scaffold
    n = len(pairs[0])
    assert 500 < int(ref.mask(pairs).sum()) < n - 500
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        whole = _same_store(ctx, pairs, len(sizes), form)
        ctx.pairs_drop()
        ctx.pairs_begin(sizes)
        at = 0
        for step in (1, 7, SLICE, n):
            ctx.pairs_add(*(a[at:at + step] for a in pairs))
            at += step
            _same_store(ctx, tuple(a[:at] for a in pairs), len(sizes), form)
        ctx.pairs_add(*(a[:0] for a in pairs))                                   # no pair: nothing changes
        parts = _same_store(ctx, pairs, len(sizes), form)
        if form == "default":
            assert all(a.tobytes() == b.tobytes() for a, b in zip(whole, parts))


@pytest.mark.parametrize("form", FORM_NAMES)
def test_slices_whose_intra_pairs_all_fall_on_one_scaffold(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = ge._scaffolds()
    rng = np.random.default_rng(11)
    n = 2 * SLICE + 300
    s = int(np.flatnonzero(sizes == 70000)[0])
    sa = np.full(n, s, np.int32)
    sb = sa.copy()
    sb[rng.random(n) < 0.02] = int(np.flatnonzero(sizes == 3007)[0])             # a few kept pairs among them
    pairs = (sa, rng.integers(1, 70001, n), sb, np.where(sb == s, rng.integers(1, 70001, n), rng.integers(1, 3008, n)))
    counts = ref.intra(pairs, len(sizes))
    assert int(counts[s]) > 2 * SLICE and int(counts.sum()) == int(counts[s])
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        _same_store(ctx, pairs, len(sizes), form)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_scaffolds_of_2_to_the_33_and_positions_above_2_to_the_32(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    L = 2 ** 33
    sizes = np.array([L, L + 1, L, 5], dtype=np.int64)
    rng = np.random.default_rng(2)
    n = 1000
    sa, sb = rng.integers(0, 4, n), rng.integers(0, 4, n)
    edge = np.array([1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, L - 1, L])
    pa = np.minimum(np.where(rng.random(n) < 0.5, rng.choice(edge, n), rng.integers(2 ** 32, L + 1, n)), sizes[sa])
    pb = np.minimum(np.where(rng.random(n) < 0.5, rng.choice(edge, n), rng.integers(2 ** 32, L + 1, n)), sizes[sb])
    pairs = (sa.astype(np.int32), pa, sb.astype(np.int32), pb)
    kept = ref.keep(pairs)
    assert int((kept[1] > 2 ** 32).sum()) > 100 and int((kept[3] > 2 ** 32).sum()) > 100
    tables = lref.layout([[(0, "+"), (1, "-"), (2, "+")]], sizes, 100, drop_unplaced=True)
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        _same_store(ctx, pairs, len(sizes), form)
        for window in (2 ** 20, 2 ** 32 + 1):
            rank, T, counters = ctx.ends_resident(sizes, *tables, window, 2)
            wT, wc = eref.table(pairs, sizes, tables, window, 2)
            assert T.tobytes() == wT.tobytes() and counters.tolist() == wc.tolist() and rank.tolist() == [0, 1, 2, -1]


@pytest.mark.parametrize("form", FORM_NAMES)
def test_the_store_is_intact_across_each_growth(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = ge._scaffolds()
    pairs = _patterned(2000, "all", seed=9)
    _set_form(monkeypatch, form)
    monkeypatch.setenv("HICMI_PAIRS_FIRST_PAIRS", "256")
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        monkeypatch.setenv("HICMI_PAIRS_FIRST_PAIRS", "1000000")                  # read per begin: this store started at 256
        for at in range(0, 2000, 100):                                           # the capacity passes 256, 512, 1024 and 2048
            ctx.pairs_add(*(a[at:at + 100] for a in pairs))
            _same_store(ctx, tuple(a[:at + 100] for a in pairs), len(sizes), form)
        ctx.pairs_drop()
        monkeypatch.setenv("HICMI_PAIRS_FIRST_PAIRS", "256")
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)                                                    # one call past the first capacity
        _same_store(ctx, pairs, len(sizes), form)
        ctx.pairs_drop()
        monkeypatch.setenv("HICMI_PAIRS_FIRST_PAIRS", "0")
        with pytest.raises(_lib.HicmiError) as exc:
            ctx.pairs_begin(sizes)
        assert "HICMI_PAIRS_FIRST_PAIRS" in str(exc.value)


# ---- the resident calls ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("count_form", ["default", "plain"])
def test_ends_resident_equals_ends_file_and_the_reference(count_form, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = ge._scaffolds()
    data, stats, tables, want, pairs = ge._odd_file()
    path = ge._write(tmp_path, data)
    _set_form(monkeypatch, form)
    if count_form == "plain":
        monkeypatch.setenv("HICMI_ENDS_PLAIN", "1")
    with _lib.Context(0) as ctx:
        got_stats = ctx.pairs_file(path, names, sizes, threads=2)
        assert got_stats[:4] == stats
        ge._same(ctx.ends_resident(sizes, *tables, WINDOW, REACH), want)
        _stats, rank, T, counters = _lib.ends_file(path, names, sizes, *tables, WINDOW, REACH, ctx, threads=2)
        ge._same((rank, T, counters), want)
        for drop in (False, True):                                               # other lift tables on the same store
            for window, reach in ((1, 1), (10 ** 9, 64)):
                other = ge._tables(0, drop)
                ge._same(ctx.ends_resident(sizes, *other, window, reach), ge._want(pairs, sizes, other, window, reach))


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("mode", ga.MODES)
def test_anchor_resident_equals_anchor_file_and_the_reference(mode, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = ga._scaffolds()
    data, stats, pairs = ga._odd_file()
    tables, target = ga._tables(), ga._target(mode)
    path = ga._write(tmp_path, data)
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        assert ctx.pairs_file(path, names, sizes)[:4] == stats
        for window in (ga.WINDOW, 1, 10 ** 6):
            want = ga._want(pairs, sizes, tables, target, window)
            ga._same(ctx.anchor_resident(sizes, *tables, target, window), want)
        ga._same(_lib.anchor_file(path, names, sizes, *tables, target, ga.WINDOW, ctx, threads=2)[1:],
                 ga._want(pairs, sizes, tables, target, ga.WINDOW))
        monkeypatch.setenv("HICMI_ANCHOR_PLAIN", "1")
        ga._same(ctx.anchor_resident(sizes, *tables, target, ga.WINDOW), ga._want(pairs, sizes, tables, target, ga.WINDOW))


@pytest.mark.parametrize("form", FORM_NAMES)
def test_three_calls_with_a_scaffold_flipped_between_them_leave_the_store_unchanged(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = ge._scaffolds()
    pairs = ge._pool()
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        before = _same_store(ctx, pairs, len(sizes), form)
        chroms = [list(ch) for ch in ge.CHROMS]
        seen = set()
        for flip in (None, (0, 3), (1, 2)):
            if flip:
                q, k = flip
                s, o = chroms[q][k]
                chroms[q][k] = (s, "+" if o == "-" else "-")
            tables = lref.layout(chroms, sizes, 100, drop_unplaced=True)
            want = ge._want(pairs, sizes, tables, WINDOW, REACH)
            got = ctx.ends_resident(sizes, *tables, WINDOW, REACH)
            ge._same(got, want)
            seen.add(got[1].tobytes())
        assert len(seen) == 3                                                    # the flips moved counts
        after = ctx.pairs_fetch()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        _same_store(ctx, pairs, len(sizes), form)


def _raw_resident(ctx, sizes, tables, window, reach, target, shapes):
    """hicmi_ends_resident (target False) or hicmi_anchor_resident (target None or an array) called raw on outputs of
    ``shapes`` filled with marks: (rc, table, counters, per scaffold output, n_out, message)."""
    from hic_genome_assembler_amd import _lib
    lib = _lib.load()
    size, seq, loff, rev, seq_size = _lib._lift_tables(sizes, *tables)
    table, counters = np.full(shapes[0], 77, np.uint64), np.full(6, 77, np.uint64)
    n_out = ctypes.c_int64(-7)
    if target is False:
        per = np.full(shapes[1], -7, np.int32)
        rc = lib.hicmi_ends_resident(ctx._h, _lib._ptr(size), len(size), _lib._ptr(seq), _lib._ptr(loff), _lib._ptr(rev), _lib._ptr(seq_size),
                                     len(seq_size), window, reach, _lib._ptr(table), _lib._ptr(counters), _lib._ptr(per), ctypes.byref(n_out))
    else:
        per = np.full(shapes[1], -7, np.int64)
        tgt = None if target is None else np.ascontiguousarray(target, dtype=np.int32)
        rc = lib.hicmi_anchor_resident(ctx._h, _lib._ptr(size), len(size), _lib._ptr(seq), _lib._ptr(loff), _lib._ptr(rev), _lib._ptr(seq_size),
                                       len(seq_size), _lib._ptr(tgt), window, _lib._ptr(table), _lib._ptr(counters), _lib._ptr(per),
                                       ctypes.byref(n_out))
    return rc, table, counters, per, n_out.value, lib.hicmi_last_error().decode()


def _unwritten(got):
    _rc, table, counters, per, n_out, _message = got
    return n_out == -7 and (table == 77).all() and (counters == 77).all() and (per == -7).all()


@pytest.mark.parametrize("form", FORM_NAMES)
def test_the_raw_resident_calls_return_n_placed_and_n_table_and_write_nothing_when_refused(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _names, sizes = ge._scaffolds()
    tables, pairs = ga._tables(), ga._pool()
    S = len(sizes)
    ends_want = ge._want(pairs, sizes, tables, WINDOW, REACH)
    n_placed = eref.number_ranks(sizes, tables)[2]
    assert ends_want[1].shape == (n_placed, REACH, 4) and 1 < n_placed < S
    ends_shapes = (ends_want[1].shape, S)
    _set_form(monkeypatch, form)
    with _lib.Context(0) as ctx:
        # no store
        for got in (_raw_resident(ctx, sizes, tables, WINDOW, REACH, False, ends_shapes),
                    _raw_resident(ctx, sizes, tables, ga.WINDOW, 0, None, (10, S))):
            assert got[0] == EINVAL and "without a pair store" in got[5] and _unwritten(got)
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        # the store answers: rank, table, counters and n_placed as the reference has them
        rc, table, counters, rank, got_placed, _message = _raw_resident(ctx, sizes, tables, WINDOW, REACH, False, ends_shapes)
        assert rc == 0 and got_placed == n_placed
        ge._same((rank, table, counters), ends_want)
        for mode in ga.MODES:
            target = ga._target(mode)
            want = ga._want(pairs, sizes, tables, target, ga.WINDOW)
            n_table = aref.number_blocks(sizes, tables, target)[1]
            assert n_table == len(want[1]) > 0
            rc, table, counters, first, got_table, _message = _raw_resident(ctx, sizes, tables, ga.WINDOW, 0, target, (n_table, S))
            assert rc == 0 and got_table == n_table
            ga._same((first, table, counters), want)
        # refused with a store: other sizes, bad parameters, an open build of the call's kind - every output stays as it was
        other = np.array(sizes)
        other[3] += 1
        anchor_shapes = (aref.number_blocks(sizes, tables, None)[1], S)
        for got, word in ((_raw_resident(ctx, other, tables, WINDOW, REACH, False, ends_shapes), "sizes"),
                          (_raw_resident(ctx, other, tables, ga.WINDOW, 0, None, anchor_shapes), "sizes"),
                          (_raw_resident(ctx, sizes, tables, 0, REACH, False, ends_shapes), "window"),
                          (_raw_resident(ctx, sizes, tables, WINDOW, 65, False, ends_shapes), "reach"),
                          (_raw_resident(ctx, sizes, tables, 0, 0, None, anchor_shapes), "window"),
                          (_raw_resident(ctx, sizes, tables, ga.WINDOW, 0, np.full(S, -1, np.int32), anchor_shapes), "no candidate")):
            assert got[0] == EINVAL and word in got[5] and _unwritten(got), got[5]
        ctx.ends_begin(sizes, *tables, WINDOW, REACH)
        ctx.anchor_begin(sizes, *tables, None, ga.WINDOW)
        got = _raw_resident(ctx, sizes, tables, WINDOW, REACH, False, ends_shapes)
        assert got[0] == EINVAL and "ends build is open" in got[5] and _unwritten(got)
        got = _raw_resident(ctx, sizes, tables, ga.WINDOW, 0, None, anchor_shapes)
        assert got[0] == EINVAL and "anchor build is open" in got[5] and _unwritten(got)
        ctx.ends_finish()
        ctx.anchor_finish()
        _same_store(ctx, pairs, S, form)


# ---- the one-pass load ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("threads", [1, 0])
@pytest.mark.parametrize("chunk", ["1000", None])
def test_pairs_file_equals_the_array_calls(chunk, threads, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = ge._scaffolds()
    data, stats, _tables, _want, pairs = ge._odd_file()
    path = ge._write(tmp_path, data)
    _set_form(monkeypatch, form)
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held + held.T)
        got_stats = _lib.pairs_file(path, names, sizes, ctx, threads=threads)
        assert got_stats[:4] == stats and got_stats[4] == (-(-stats[1] // 1000) if chunk else 1) and stats[1] > 4 * 1000
        from_file = _same_store(ctx, pairs, len(sizes), form)
        assert ctx.n == 4 and ctx.contacts_host().tobytes() == (held + held.T).tobytes()
        ctx.pairs_drop()
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        from_arrays = _same_store(ctx, pairs, len(sizes), form)
        if form == "default":
            assert all(a.tobytes() == b.tobytes() for a, b in zip(from_file, from_arrays))


@pytest.mark.parametrize("chunk", ["100", "1000", None])
def test_a_malformed_line_leaves_no_store_and_untouched_outputs(chunk, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = ge._scaffolds()
    data, stats, _tables, _want, pairs = ge._odd_file()
    _set_form(monkeypatch, "default")
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    lib = _lib.load()
    blob, off = _lib._name_blob(names)
    size = np.ascontiguousarray(sizes, dtype=np.int64)
    # the bad line lies mid-file: more than 3,000 good pairs before it - with a chunk setting they are in the store when the
    # parser meets it - and as many good lines after it
    cut = data.index(b"\n", len(data) // 2) + 1
    before = bref.parse_text(data[:cut], names, sizes)[1]
    assert before[1] > 3000 and stats[1] - before[1] > 3000
    bad = ge._write(tmp_path, data[:cut] + b"read\tscaffold_4\t12x\t+\tscaffold_4\t5\n" + data[cut:])
    with _lib.Context(0) as ctx:
        out = np.full(5, -7, np.int64)
        rc = lib.hicmi_pairs_file(os.fsencode(bad), blob, _lib._ptr(off), len(names), _lib._ptr(size), ctx._h, 2, _lib._ptr(out))
        assert rc == EINVAL and lib.hicmi_last_error().decode().endswith("at byte %d" % cut) and (out == -7).all()
        n_kept, n_intra = ctypes.c_int64(-7), ctypes.c_uint64(7)
        assert lib.hicmi_pairs_info(ctx._h, ctypes.byref(n_kept), ctypes.byref(n_intra), None) == EINVAL      # no store is left
        assert n_kept.value == -7 and n_intra.value == 7
        rc = lib.hicmi_pairs_file(os.fsencode(str(tmp_path / "missing")), blob, _lib._ptr(off), len(names), _lib._ptr(size), ctx._h, 2,
                                  _lib._ptr(out))
        assert rc == EINVAL and "cannot open" in lib.hicmi_last_error().decode() and (out == -7).all()
        good = ge._write(tmp_path, data)
        assert ctx.pairs_file(good, names, sizes)[:4] == stats                    # the context takes a store afterwards
        assert lib.hicmi_pairs_info(ctx._h, ctypes.byref(n_kept), ctypes.byref(n_intra), None) == 0           # intra_out may be NULL
        assert n_kept.value == int(ref.mask(pairs).sum()) and n_kept.value + n_intra.value == stats[1]
        rc = lib.hicmi_pairs_file(os.fsencode(good), blob, _lib._ptr(off), len(names), _lib._ptr(size), ctx._h, 2, _lib._ptr(out))
        assert rc == EINVAL and "already" in lib.hicmi_last_error().decode() and (out == -7).all()
        _same_store(ctx, pairs, len(sizes), "default")                           # the refused load left the store as it was


# ---- misuse ----------------------------------------------------------------------------------------------------------------------------
def test_misuse_leaves_the_store_the_matrix_and_the_open_builds_as_they_were(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    _names, sizes = ge._scaffolds()
    tables, target = ga._tables(), ga._target("rank")
    pairs = ga._pool()
    n = len(pairs[0])
    half = n // 2
    map_want = bref.build(pairs, sizes, bref.R)
    span_recs = [(0, 10, 0, int(sref.number_cells(sizes, tables, 500)[1][1]))]
    span_D, span_counters, _marks = sref.depth(pairs, sizes, tables, 500)
    span_picks = sref.picks(span_D, 3, span_recs)
    ends_want = ge._want(pairs, sizes, tables, WINDOW, REACH)
    anchor_want = ga._want(pairs, sizes, tables, target, ga.WINDOW)
    held = np.arange(25, dtype=np.float64).reshape(5, 5)
    held = held + held.T

    def refused(call, word=None):
        with pytest.raises(_lib.HicmiError) as exc:
            call()
        assert "error %d:" % EINVAL in str(exc.value) and (word is None or word in str(exc.value)), str(exc.value)

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
        ctx.map_begin(sizes, bref.R)                                          # a map, a span, an ends and an anchor build stay open
        ctx.map_add_pairs(*ge._first(pairs, half))
        ctx.span_begin(sizes, *tables, 500)
        ctx.span_add_pairs(*ge._first(pairs, half))
        rank = ctx.ends_begin(sizes, *tables, WINDOW, REACH)
        ctx.ends_add_pairs(*ge._first(pairs, half))
        first = ctx.anchor_begin(sizes, *tables, target, ga.WINDOW)
        ctx.anchor_add_pairs(*ge._first(pairs, half))
        # no store
        refused(lambda: ctx.ends_resident(sizes, *tables, WINDOW, REACH), word="without a pair store")
        refused(lambda: ctx.anchor_resident(sizes, *tables, target, ga.WINDOW), word="without a pair store")
        refused(lambda: ctx.pairs_add(*pairs), word="without")
        refused(lambda: ctx.pairs_info(), word="without")
        refused(lambda: ctx.pairs_drop(), word="without")
        refused(lambda: ctx.pairs_begin(changed(sizes, 3, -1)), word="scaffold 3 ")
        refused(lambda: ctx.pairs_info(), word="without")                        # the refused begin opened nothing
        ctx.pairs_begin(sizes)
        refused(lambda: ctx.pairs_begin(sizes), word="already")
        ctx.pairs_add(*ge._first(pairs, 1000))
        # an out-of-range pair is refused with the store as before
        refused(lambda: ctx.pairs_add(changed(sa, 200, len(sizes)), pa, sb, pb), word="pair 200 ")
        refused(lambda: ctx.pairs_add(sa, pa, sb, changed(pb, 100, sizes[sb[100]] + 1)), word="pair 100 ")
        refused(lambda: ctx.pairs_add(sa, changed(pa, 4000, 0), sb, pb), word="pair 4000 ")
        _same_store(ctx, ge._first(pairs, 1000), len(sizes), "default")
        ctx.pairs_add(*(a[1000:] for a in pairs))
        store = _same_store(ctx, pairs, len(sizes), "default")
        # the resident calls while a build of their kind is open, and with other scaffold sizes
        refused(lambda: ctx.ends_resident(sizes, *tables, WINDOW, REACH), word="ends build is open")
        refused(lambda: ctx.anchor_resident(sizes, *tables, target, ga.WINDOW), word="anchor build is open")
        ctx.ends_add_pairs(*(a[half:] for a in pairs))                         # the builds still finish with the right tables
        ge._same((rank,) + ctx.ends_finish(), ends_want)
        ctx.anchor_add_pairs(*(a[half:] for a in pairs))
        ga._same((first,) + ctx.anchor_finish(), anchor_want)
        refused(lambda: ctx.ends_resident(changed(sizes, 3, sizes[3] + 1), *tables, WINDOW, REACH), word="sizes")
        refused(lambda: ctx.ends_resident(sizes[:-1], tables[0][:-1], tables[1][:-1], tables[2][:-1], tables[3], WINDOW, REACH), word="sizes")
        refused(lambda: ctx.anchor_resident(changed(sizes, 3, sizes[3] + 1), *tables, target, ga.WINDOW), word="sizes")
        refused(lambda: ctx.ends_resident(sizes, *tables, 0, REACH), word="window")
        refused(lambda: ctx.ends_resident(sizes, *tables, WINDOW, 65), word="reach")
        refused(lambda: ctx.anchor_resident(sizes, *tables, np.full(40, -1, np.int32), ga.WINDOW), word="no candidate")
        refused(lambda: ctx.ends_finish(), word="without")                       # no refused call left a build open
        refused(lambda: ctx.anchor_finish(), word="without")
        ge._same(ctx.ends_resident(sizes, *tables, WINDOW, REACH), ends_want)
        ga._same(ctx.anchor_resident(sizes, *tables, target, ga.WINDOW), anchor_want)
        refused(lambda: ctx.ends_finish(), word="without")                       # ... nor did the ones that answered
        refused(lambda: ctx.anchor_finish(), word="without")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(store, ctx.pairs_fetch()))
        untouched(ctx)
        # the span build and the map build that were open all the while are what they would have been
        ctx.span_add_pairs(*(a[half:] for a in pairs))
        picks, counters, depth = ctx.span_finish(3, span_recs)
        assert depth.tobytes() == span_D.tobytes() and counters.tolist() == span_counters.tolist() and picks.tolist() == span_picks.tolist()
        ctx.map_add_pairs(*(a[half:] for a in pairs))
        assert ctx.map_finish() == n and ctx.contacts_host().tobytes() == map_want.tobytes()
        _same_store(ctx, pairs, len(sizes), "default")
    ctx = _lib.Context(0)                                                     # a context destroyed with its store
    ctx.pairs_begin(sizes)
    ctx.pairs_add(*pairs)
    ctx.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_cli_round_trip_of_the_mixed_planted_case(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import polishOrder
    import test_polish_cpu as cpu
    _set_form(monkeypatch, "default")
    cfg, order, _save = cpu.mixed_files(tmp_path)
    on_device, on_stand_in = str(tmp_path / "device"), str(tmp_path / "stand_in")
    status, rounds, _log = polishOrder.main(["-config", cfg, "-order", order, "-window", "5000", "-out", on_device, "-threads", "3"])
    assert status == "converged" and "POLISH: converged after %d round(s)" % rounds in capsys.readouterr().out
    polishOrder.main(["-config", cfg, "-order", order, "-window", "5000", "-out", on_stand_in], context=ref.StandInContext())
    for name in (os.path.basename(order), "polish.log", "polish_summary.tsv"):
        assert cpu._read(os.path.join(on_device, name)) == cpu._read(os.path.join(on_stand_in, name)), name
    cpu.check_mixed_outputs(cpu._read(os.path.join(on_device, os.path.basename(order))))
