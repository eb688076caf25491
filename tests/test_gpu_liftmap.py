"""Maps of the assembled genome counted on the device (hicmi_map_begin_lifted, hicmi_pair_stats, hicmi_lift_maps;
DESIGN.md 9m) against tests/liftmap_reference.py, for HICMI_LIFTMAP_PLAIN unset, =1 and =0, byte for byte - the counts
and the statistics are integers, there are no tolerances: the identity lift against a plain build, real lifts with
gaps, junction bins, 64-bit coordinates, hot cells and counters, chunking, misuse, the one-pass driver, and
assembledMap's files."""
import functools
import os

import numpy as np
import pytest

import buildmap_reference as bref
import liftmap_reference as ref

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -5
# Both counting forms give the same bytes by design, so these tests hold each form to the reference but cannot tell which
# kernel a setting launched; that the switch is read (per call, by its own name) is checked from the source in the CPU file.
FORMS = {"default": {}, "plain": {"HICMI_LIFTMAP_PLAIN": "1"}, "combine": {"HICMI_LIFTMAP_PLAIN": "0"}}
FORM_NAMES = ["default", "plain", "combine"]
R = ref.R
# slices that end inside, on and just past a wave (64), a workgroup (256), the pairs one workgroup of the statistics kernel
# brings together (1024) and those of the combining kernel (2048)
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5001]
# three chromosomes of mixed orientations on the 40 odd scaffolds; 20 scaffolds stay unplaced
CHROMS = [[(3, "+"), (0, "-"), (4, "-"), (17, "+"), (1, "-"), (2, "+"), (7, "-")],
          [(38, "-"), (5, "-"), (6, "+"), (9, "-"), (8, "+"), (11, "+"), (12, "-"), (13, "-")],
          [(20, "-"), (21, "+"), (22, "-"), (24, "+"), (23, "-")]]


def _set_form(monkeypatch, form):
    for key in ("HICMI_LIFTMAP_PLAIN", "HICMI_BUILDMAP_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS"):
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
def _pool(n):
    names, sizes = _scaffolds()
    return _frozen(*(a[:n] for a in bref.edge_pairs(names, sizes, COUNTS[-1], seed=7)))


@functools.lru_cache(maxsize=None)
def _tables(gap, drop):
    """The lift tables of CHROMS; they must hold the cases the kernels have to get right."""
    _names, sizes = _scaffolds()
    seq, off, rev, seq_sizes = ref.layout(CHROMS, sizes, gap, drop_unplaced=drop)
    assert len(seq_sizes) == (3 if drop else 23) and (seq == -1).sum() == (20 if drop else 0) and rev.sum() == 12
    assert any(sizes[s] == 1 and rev[s] for s in range(40))                          # a size-1 scaffold reversed
    # junctions inside a bin: the bins of the chromosomes are not the scaffolds' bins laid end to end
    placed = seq_sizes[:3]
    assert bref.first_bins(placed, R)[1] < bref.first_bins(sizes[(seq >= 0) & (seq < 3)], R)[1]
    return _frozen(seq, off, rev, seq_sizes)


@functools.lru_cache(maxsize=None)
def _want(n, gap, drop, r):
    """(reference map, reference statistics as arrays, pairs lifted) of the first n pool pairs."""
    _names, sizes = _scaffolds()
    dense, stats = ref.build(_pool(n), sizes, _tables(gap, drop), r)
    arrays = ref.stats_arrays(stats)
    if n == COUNTS[-1]:                                      # the whole pool: cis and trans pairs, many distances, lost pairs
        decay, cis, trans, unlifted = arrays
        assert cis.sum() > 200 and trans.sum() > 200 and trans.sum() // 2 + cis.sum() + unlifted[0] == n
        assert decay.sum() == cis.sum() and decay[0] > 0 and np.count_nonzero(decay) > 20
        assert (unlifted[0] > 1000) == drop and (unlifted[0] > 0) == drop
    _frozen(dense, *arrays)
    return dense, arrays, n - stats[3]


def _count(sizes, tables, r, parts, lifted=True):
    """(map, pairs returned by finish, both row sums) after one add call per element of ``parts``."""
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        if lifted:
            ctx.map_begin_lifted(sizes, *tables, r)
        else:
            ctx.map_begin(sizes, r)
        for p in parts:
            ctx.map_add_pairs(*p)
        n = ctx.map_finish()
        return ctx.contacts_host(), n, ctx.row_sums()


def _stats(sizes, tables, parts):
    from hic_genome_assembler_amd import _lib
    into = _lib.new_pair_stats(len(tables[3]))
    with _lib.Context(0) as ctx:
        for p in parts:
            assert ctx.pair_stats(*p, sizes, *tables, into=into) is into
    return into


def _same_stats(got, want):
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == np.uint64 and g.shape == w.shape and g.tobytes() == w.tobytes()


def _check_map(got, n, sums, want, pairs_lifted):
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert n == pairs_lifted == np.triu(got).sum()
    # both row sums of the context (two summation orders; integers, so exact), against the rows and the columns of the map
    assert np.array_equal(sums[0], want.sum(axis=1)) and np.array_equal(sums[1], want.sum(axis=0))


# ---- the identity lift is a plain build ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _identity_want(n):
    _names, sizes = _scaffolds()
    tables = _frozen(*ref.identity(sizes))
    dense, stats = ref.build(_pool(n), sizes, tables, R)
    assert dense.tobytes() == bref.build(_pool(n), sizes, R).tobytes() and dense.shape == (277, 277)
    return tables, _frozen(dense)[0], _frozen(*ref.stats_arrays(stats))


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("n", COUNTS)
def test_identity_lift_equals_a_plain_build_bit_for_bit(n, form, monkeypatch):
    _names, sizes = _scaffolds()
    tables, want, want_stats = _identity_want(n)
    _set_form(monkeypatch, form)
    plain, n_plain, _sums = _count(sizes, None, R, [_pool(n)], lifted=False)
    got, n_got, sums = _count(sizes, tables, R, [_pool(n)])
    assert got.tobytes() == plain.tobytes() and n_got == n_plain == n
    _check_map(got, n_got, sums, want, n)
    _same_stats(_stats(sizes, tables, [_pool(n)]), want_stats)


# ---- a real lift ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", [0, 1, 100])
def test_three_chromosomes_of_mixed_orientations(gap, drop, form, monkeypatch):
    _names, sizes = _scaffolds()
    tables = _tables(gap, drop)
    pairs = _pool(COUNTS[-1])
    _set_form(monkeypatch, form)
    for r in (R, 2 * R + 1, 10 ** 7):                        # the last: one bin per sequence
        want, want_stats, lifted = _want(COUNTS[-1], gap, drop, r)
        got, n, sums = _count(sizes, tables, r, [pairs])
        _check_map(got, n, sums, want, lifted)
        assert r < 10 ** 7 or len(got) == len(tables[3])
    got_stats = _stats(sizes, tables, [pairs])
    _same_stats(got_stats, want_stats)
    assert int(got_stats[3][0]) == COUNTS[-1] - lifted and (int(got_stats[3][0]) > 0) == drop


@pytest.mark.parametrize("form", FORM_NAMES)
def test_three_calls_equal_one_and_the_sums_accumulate(form, monkeypatch):
    _names, sizes = _scaffolds()
    tables = _tables(100, True)
    pairs = _pool(COUNTS[-1])
    want, want_stats, lifted = _want(COUNTS[-1], 100, True, R)
    _set_form(monkeypatch, form)
    cuts = [0, 100, 2500, COUNTS[-1]]
    parts = [tuple(a[cuts[k]:cuts[k + 1]] for a in pairs) for k in range(3)] + [tuple(a[:0] for a in pairs)]
    got, n, sums = _count(sizes, tables, R, parts)
    _check_map(got, n, sums, want, lifted)
    _same_stats(_stats(sizes, tables, parts), want_stats)
    # a second round of calls adds to what is there
    from hic_genome_assembler_amd import _lib
    twice = _stats(sizes, tables, [pairs])
    with _lib.Context(0) as ctx:
        ctx.pair_stats(*pairs, sizes, *tables, into=twice)
    _same_stats(twice, tuple(w * np.uint64(2) for w in want_stats))


# ---- junction bins ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("gap", [0, 100])
def test_junctions_inside_a_bin(gap, form, monkeypatch):
    """Scaffolds of 1,500, 700 and 2,300 bp at r = 1,000: both junctions fall inside a bin, and the last base of one scaffold
    and the first of the next (in the assembly's direction) are counted in one bin."""
    sizes = np.array([1500, 700, 2300], dtype=np.int64)
    tables = ref.layout([[(0, "+"), (1, "-"), (2, "+")]], sizes, gap)
    #        last of 0 / first of 1 (reversed: its base 700)   last of 1 (its base 1) / first of 2    far ends
    pairs = (np.array([0, 1, 1, 2, 0, 2, 0, 1], np.int32), np.array([1500, 700, 1, 1, 1, 2300, 1500, 1], np.int64),
             np.array([1, 0, 2, 1, 2, 0, 0, 1], np.int32), np.array([700, 1500, 1, 1, 2300, 1, 1400, 700], np.int64))
    lifted, _stats_ref = ref.lift_and_stats(pairs, sizes, tables)
    assert lifted[1][0] == 1500 and lifted[3][0] == 1501 + gap and lifted[1][2] == 2200 + gap and lifted[3][2] == 2201 + 2 * gap
    want, stats = ref.build(pairs, sizes, tables, 1000)
    assert len(want) == -(-(4500 + 2 * gap) // 1000) and want[1, 1] >= 3 and want[2, 2] >= 2
    _set_form(monkeypatch, form)
    got, n, sums = _count(sizes, tables, 1000, [pairs])
    _check_map(got, n, sums, want, 8)
    _same_stats(_stats(sizes, tables, [pairs]), ref.stats_arrays(stats))


# ---- 64-bit coordinates -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
def test_three_scaffolds_of_2_to_the_33(form, monkeypatch):
    L = 2 ** 33
    sizes = np.array([L, L, L], dtype=np.int64)
    tables = ref.layout([[(0, "+"), (1, "-"), (2, "+")]], sizes, 100)
    edge = np.array([1, 2, 2 ** 27, 2 ** 27 + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, L - 2 ** 27, L - 1, L], dtype=np.int64)
    rng = np.random.default_rng(3)
    n = 600
    sa, sb = rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32)
    pa = np.where(rng.random(n) < 0.5, rng.choice(edge, n), rng.integers(1, L + 1, n))
    pb = np.where(rng.random(n) < 0.5, rng.choice(edge, n), rng.integers(1, L + 1, n))
    pairs = (sa, pa, sb, pb)
    r = 2 ** 27
    want, stats = ref.build(pairs, sizes, tables, r)
    assert len(want) == 193 and np.count_nonzero(stats[0][120:]) > 3                 # distances beyond 2^30
    _set_form(monkeypatch, form)
    got, n_got, sums = _count(sizes, tables, r, [pairs])
    _check_map(got, n_got, sums, want, n)
    _same_stats(_stats(sizes, tables, [pairs]), ref.stats_arrays(stats))


# ---- hot cells and counters -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hot(case):
    _names, sizes = _scaffolds()
    tables = _tables(100, False)
    if case == "one_pair":                                   # 100,000 copies of one trans pair: one cell, two counters
        pairs = tuple(np.full(100000, v, dtype=t) for v, t in ((3, np.int32), (69 * R + 1, np.int64), (38, np.int32), (R, np.int64)))
    else:                                                    # 100,000 cis pairs in Chr_1: one cis counter, few decay slots
        rng = np.random.default_rng(9)
        chrom = np.array([s for s, _o in CHROMS[0]])
        sa, sb = rng.choice(chrom, 100000).astype(np.int32), rng.choice(chrom, 100000).astype(np.int32)
        pairs = (sa, 1 + np.floor(rng.random(100000) * sizes[sa]).astype(np.int64),
                 sb, 1 + np.floor(rng.random(100000) * sizes[sb]).astype(np.int64))
    want, stats = ref.build(pairs, sizes, tables, R)
    return _frozen(*pairs), tables, _frozen(want)[0], _frozen(*ref.stats_arrays(stats))


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("case", ["one_pair", "one_sequence"])
def test_hot_cells_and_counters_are_exact(case, form, monkeypatch):
    _names, sizes = _scaffolds()
    pairs, tables, want, want_stats = _hot(case)
    decay, cis, trans, unlifted = want_stats
    if case == "one_pair":
        assert want.max() == 100000 and np.count_nonzero(want) == 2 and trans[0] == trans[1] == 100000 and cis.sum() == 0
    else:
        assert cis[0] == 100000 == decay.sum() and cis[1:].sum() == 0 and trans.sum() == 0 and decay.max() > 10000
    _set_form(monkeypatch, form)
    got, n, sums = _count(sizes, tables, R, [pairs])
    _check_map(got, n, sums, want, 100000)
    _same_stats(_stats(sizes, tables, [pairs]), want_stats)


# ---- misuse -----------------------------------------------------------------------------------------------------------------------
def test_misuse_leaves_the_matrix_and_a_later_build_right(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    _names, sizes = _scaffolds()
    tables = _tables(100, True)
    seq, off, rev, seq_sizes = tables
    pairs = _pool(257)
    want, _stats_want, lifted = _want(257, 100, True, R)
    plain_want = bref.build(pairs, sizes, R)
    held = np.arange(25, dtype=np.float64).reshape(5, 5)
    held = held + held.T

    def refused(call, code=EINVAL, word=None):
        with pytest.raises(_lib.HicmiError) as exc:
            call()
        assert "error %d:" % code in str(exc.value) and (word is None or word in str(exc.value)), str(exc.value)

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out

    bad_tables = [((changed(seq, 7, len(seq_sizes)), off, rev, seq_sizes), "scaffold 7 "),
                  ((changed(seq, 7, -2), off, rev, seq_sizes), "scaffold 7 "),
                  ((seq, changed(off, 4, -1), rev, seq_sizes), "scaffold 4 "),
                  ((seq, changed(off, 7, seq_sizes[0] - sizes[7] + 1), rev, seq_sizes), "scaffold 7 "),
                  ((seq, changed(off, 4, off[17]), rev, seq_sizes), "overlap"),
                  ((seq, off, rev, changed(seq_sizes, 1, seq_sizes[1] - 1)), "scaffold ")]
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held)
        for bad, word in bad_tables:
            refused(lambda: ctx.map_begin_lifted(sizes, *bad, R), word=word)
            refused(lambda: ctx.pair_stats(*pairs, sizes, *bad), word=word)
        refused(lambda: ctx.map_begin_lifted(sizes, *tables, 0))
        refused(lambda: ctx.map_begin_lifted([65537 * 10], [0], [0], [0], [65537 * 10], 10), EUNSUPPORTED)
        with pytest.raises(ValueError):
            ctx.map_begin_lifted(sizes, seq[:5], off, rev, seq_sizes, R)
        refused(lambda: ctx.map_add_pairs(*pairs))           # none of them opened a build
        refused(ctx.map_finish)
        assert ctx.n == 5 and ctx.contacts_host().tobytes() == held.tobytes()
        # a failed begin_lifted leaves an open build open, and add_pairs checks against the scaffold sizes
        ctx.map_begin_lifted(sizes, *tables, R)
        refused(lambda: ctx.map_begin_lifted(sizes, *bad_tables[0][0], R))
        sa, pa, sb, pb = pairs
        refused(lambda: ctx.map_add_pairs(changed(sa, 200, len(sizes)), pa, sb, pb))
        refused(lambda: ctx.map_add_pairs(sa, pa, sb, changed(pb, 100, sizes[sb[100]] + 1)))
        refused(lambda: ctx.pair_stats(sa, changed(pa, 256, 0), sb, pb, sizes, *tables))
        assert ctx.n == 5 and ctx.contacts_host().tobytes() == held.tobytes()
        assert np.array_equal(ctx.row_sums()[0], held.sum(axis=1))
        ctx.map_add_pairs(*pairs)
        assert ctx.map_finish() == lifted < 257 and ctx.contacts_host().tobytes() == want.tobytes()
        # a plain build after a lifted one, and the reverse: nothing of the lift stays behind
        ctx.map_begin(sizes, R)
        ctx.map_add_pairs(*pairs)
        assert ctx.map_finish() == 257 and ctx.contacts_host().tobytes() == plain_want.tobytes()
        ctx.map_begin(sizes, R)
        ctx.map_add_pairs(*pairs)
        ctx.map_begin_lifted(sizes, *tables, R)              # gives the open plain build up
        ctx.map_add_pairs(*pairs)
        assert ctx.map_finish() == lifted and ctx.contacts_host().tobytes() == want.tobytes()
        ctx.map_begin_lifted(sizes, *tables, R)
        ctx.map_add_pairs(*pairs)
        ctx.map_begin(sizes, R)                              # and the reverse
        ctx.map_add_pairs(*pairs)
        assert ctx.map_finish() == 257 and ctx.contacts_host().tobytes() == plain_want.tobytes()
        refused(ctx.map_finish)
    ctx = _lib.Context(0)                                    # a context destroyed between begin and finish
    ctx.map_begin_lifted(sizes, *tables, R)
    ctx.map_add_pairs(*pairs)
    ctx.close()


# ---- the driver: one pass, several resolutions, the statistics ------------------------------------------------------------------
RESOLUTIONS = [R, R * 3 // 2]


@functools.lru_cache(maxsize=None)
def _odd_file():
    names, sizes = _scaffolds()
    data = bref.odd_file_bytes(names, sizes, 5000, seed=23)
    pairs, stats, _after = bref.parse_text(data, names, sizes)
    tables = _tables(100, True)
    maps = tuple(ref.build(pairs, sizes, tables, r)[0] for r in RESOLUTIONS)
    plain = tuple(bref.build(pairs, sizes, r) for r in RESOLUTIONS)
    want_stats = ref.stats_arrays(ref.lift_and_stats(pairs, sizes, tables)[1])
    _frozen(*(maps + plain + want_stats))
    return data, stats, tables, maps, plain, want_stats


def _write(tmp_path, data):
    path = str(tmp_path / "pairs.allValidPairs")
    with open(path, "wb") as fh:
        fh.write(data)
    return path


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("chunk", ["512", None])
def test_lift_maps_at_two_resolutions_in_one_pass(chunk, threads, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, stats, tables, maps, plain, want_stats = _odd_file()
    path = _write(tmp_path, data)
    _set_form(monkeypatch, form)
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    ctxs = [_lib.Context(0) for _r in RESOLUTIONS]
    try:
        got, got_stats = _lib.lift_maps(path, names, sizes, *tables, RESOLUTIONS, ctxs, threads=threads)
        assert got[:4] == stats
        assert got[4] == (-(-stats[1] // 512) if chunk else 1) and stats[1] > 4 * 512
        _same_stats(got_stats, want_stats)
        assert int(got_stats[3][0]) > 500
        for ctx, want in zip(ctxs, maps):
            assert ctx.n == len(want) and ctx.contacts_host().tobytes() == want.tobytes()
            assert np.array_equal(ctx.row_sums()[0], want.sum(axis=1))
            assert np.triu(want).sum() == stats[1] - int(got_stats[3][0])
        # the statistics are added to what the caller hands over
        again = _lib.lift_maps(path, names, sizes, *tables, RESOLUTIONS[:1], ctxs[:1], threads=threads, into=got_stats)[1]
        assert again is got_stats
        _same_stats(again, tuple(w * np.uint64(2) for w in want_stats))
        # hicmi_build_maps, which shares the chunk loop, still gives what it gave
        assert _lib.build_maps(path, names, sizes, RESOLUTIONS, ctxs, threads=threads) == got
        for ctx, want in zip(ctxs, plain):
            assert ctx.n == len(want) and ctx.contacts_host().tobytes() == want.tobytes()
    finally:
        for ctx in ctxs:
            ctx.close()


@pytest.mark.parametrize("chunk", ["512", None])
def test_lift_maps_error_changes_no_context(chunk, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, _stats, tables, maps, _plain, want_stats = _odd_file()
    path = _write(tmp_path, data + b"\nread\tscaffold_4\t12x\t+\tscaffold_4\t5\n")
    _set_form(monkeypatch, "default")
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    held = held + held.T
    into = _lib.new_pair_stats(len(tables[3]))
    with _lib.Context(0) as a, _lib.Context(0) as b:
        a.set_contacts(held)
        with pytest.raises(_lib.HicmiError) as exc:
            _lib.lift_maps(path, names, sizes, *tables, RESOLUTIONS, [a, b], into=into)
        assert "error %d:" % EINVAL in str(exc.value) and str(exc.value).endswith("at byte %d" % (len(data) + 1))
        assert a.n == 4 and a.contacts_host().tobytes() == held.tobytes()
        assert not any(x.any() for x in into)
        with pytest.raises(_lib.HicmiError):
            b.contacts_device()                                              # it had no matrix and has none
        for call in (a.map_finish, b.map_finish):                            # and no build is left open
            with pytest.raises(_lib.HicmiError):
                call()
        with pytest.raises(_lib.HicmiError) as exc:                          # bad tables: refused before the file is opened
            _lib.lift_maps(str(tmp_path / "missing"), names, sizes, tables[0], tables[1], tables[2], tables[3] - 1, RESOLUTIONS, [a, b])
        assert "error %d:" % EINVAL in str(exc.value) and "scaffold " in str(exc.value)
        with pytest.raises(_lib.HicmiError) as exc:
            _lib.lift_maps(str(tmp_path / "missing"), names, np.array(sizes) * 10, tables[0], tables[1] * 10, tables[2],
                           tables[3] * 10, [R, 1], [a, b])
        assert "error %d:" % EUNSUPPORTED in str(exc.value) and "resolution 1 " in str(exc.value)
        good = _write(tmp_path, data)
        _lib.lift_maps(good, names, sizes, *tables, RESOLUTIONS, [a, b], into=into)
        assert a.contacts_host().tobytes() == maps[0].tobytes() and b.contacts_host().tobytes() == maps[1].tobytes()
        _same_stats(into, want_stats)


# ---- the command line ---------------------------------------------------------------------------------------------------------------
def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_cli_round_trip(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import _lib, assembledMap, buildMap, hostio, rebinMap, synth
    from hic_genome_assembler_amd import run_hicAssembler as drv
    monkeypatch.setenv("HICMI_LOUVAIN_SEED", "0")
    for key in ("HICMI_ICE_INPLACE", "HICMI_ICE_REPARSE", "HICMI_REBIN_PLAIN", "HICMI_BUILDMAP_PLAIN", "HICMI_LIFTMAP_PLAIN",
                "HICMI_BUILDMAP_CHUNK_PAIRS"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("HICMI_NO_PLOTS", "1")
    lay = synth.make_layout(160)
    counts, lay = synth.make_raw_counts(lay)
    r = lay.resolution
    names, sizes = lay.scaffold_names, lay.scaffold_sizes_bp
    work = str(tmp_path)
    paths = synth.write_hicpro(os.path.join(work, "in"), lay, None)
    pair_file = os.path.join(work, "in", "synth.allValidPairs")
    n_pairs = synth.write_valid_pairs(pair_file, lay, counts)
    # the planted layout as an order file: the scaffolds of a chromosome by rank, flipped where planted so; the last
    # chromosome stays unplaced
    n_chrom = int(lay.scaffold_chrom.max()) + 1
    chroms = [[(int(s), "+" if lay.scaffold_orient[s] > 0 else "-")
               for s in sorted(np.flatnonzero(lay.scaffold_chrom == c).tolist(), key=lambda s: lay.scaffold_rank[s])]
              for c in range(n_chrom - 1)]
    assert any(o == "-" for ch in chroms for _s, o in ch) and any(o == "+" for ch in chroms for _s, o in ch)
    order = os.path.join(work, "orders.txt")
    with open(order, "w") as fh:
        fh.write(ref.order_file_text(chroms, names))
    cfg = synth.write_config(os.path.join(work, "config.txt"), paths, os.path.join(work, "out"), os.path.join(work, "plots"),
                             5 * r, extra={"validPairFile": pair_file})
    out = os.path.join(work, "assembled")
    assembledMap.main(["-config", cfg, "-resolution", "%d,%d" % (r, 2 * r), "-order", order, "-out", out, "-threads", "3"])
    said = capsys.readouterr().out
    assert "ASSEMBLED: lines %d, pairs used %d, unknown scaffold 0, out of range 0, chunks 1, unlifted 0" % (n_pairs, n_pairs) in said
    # the reference on the file's pairs
    pairs, _stats, _after = bref.parse_text(_read(pair_file), names, sizes)
    tables = ref.layout(chroms, sizes, 100)
    lifted, (decay, cis, trans, unlifted) = ref.lift_and_stats(pairs, sizes, tables)
    assert unlifted == 0 and sum(cis) > 0 and sum(trans) > 0
    assert "ASSEMBLED: cis %d, trans %d, cis fraction %r" % (sum(cis), sum(trans) // 2, sum(cis) / n_pairs) in said
    p1, p2 = rebinMap.output_paths(out, r, prefix="assembled"), rebinMap.output_paths(out, 2 * r, prefix="assembled")
    # (1) the sizes, and the raw maps load back equal to the reference
    seq_names, seq_sizes = hostio.read_scaffold_sizes(os.path.join(out, "assembly.sizes"))
    assert seq_sizes.tolist() == tables[3].tolist() and seq_names[:n_chrom - 1] == ["Chr_%d" % (c + 1) for c in range(n_chrom - 1)]
    assert _read(os.path.join(out, "assembly.agp")).count(b"\tW\t") == len(names)
    maps = {}
    for res, p in ((r, p1), (2 * r, p2)):
        bins = hostio.read_bed_bins(p["hicProBedFile"])
        assert [(b.chrom, b.start, b.stop, b.ID) for b in bins] == bref.bed_rows(seq_names, seq_sizes, res)
        maps[res] = hostio.read_contact_matrix(p["hicProRawMatrixFile"], bins)
        assert maps[res].tobytes() == bref.build(lifted, tables[3], res).tobytes()
        assert os.path.getsize(p["hicProMatrixFile"]) > 0 and os.path.getsize(p["hicProBiasFile"]) > 0
    # (2) the grids nest (every sequence is cut from its own start), so the 2 r map is hicmi_rebin of the r map
    _coarse, group_start = hostio.rebin_bins(hostio.read_bed_bins(p1["hicProBedFile"]), 2)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(maps[r])
        ctx.rebin(group_start)
        assert ctx.contacts_host().tobytes() == maps[2 * r].tobytes()
    # (3) the summaries
    with open(os.path.join(out, "assembled_summary.tsv")) as fh:
        summary = [ln.split("\t") for ln in fh.read().splitlines()]
    assert summary[0] == ["#lines=%d" % n_pairs, "used=%d" % n_pairs, "unknown_scaffold=0", "out_of_range=0", "unlifted=0"]
    assert summary[1][0] == "#resolution" and len(summary) == 4 and len(summary[2]) == len(summary[3]) == 10
    assert summary[2][:2] == [str(r), str(len(maps[r]))] and float(summary[2][9]) == float(summary[3][9]) == n_pairs
    with open(os.path.join(out, "assembly_stats.tsv")) as fh:
        rows = [ln.split("\t") for ln in fh.read().splitlines()]
    assert len(rows) == len(seq_names) + 2 and rows[0][0] == "#sequence"
    for q, row in enumerate(rows[1:-1]):
        assert row[:5] == [seq_names[q], str(seq_sizes[q]), str(int((tables[0] == q).sum())), str(cis[q]), str(trans[q])]
        assert row[5] == (repr(cis[q] / (cis[q] + trans[q])) if cis[q] + trans[q] else "NA")
    assert rows[-1] == ["total", str(int(seq_sizes.sum())), str(len(names)), str(sum(cis)), str(sum(trans) // 2), repr(sum(cis) / n_pairs)]
    with open(os.path.join(out, "decay.tsv")) as fh:
        lines = [ln.split("\t") for ln in fh.read().splitlines()][1:]
    assert [int(ln[2]) for ln in lines] == [c for c in decay if c] and len(lines) > 20
    for (lo, hi, _count), slot in zip(lines, [k for k, c in enumerate(decay) if c]):
        assert ref.slot(int(lo)) == ref.slot(int(hi)) == slot and (int(lo) == 0 or ref.slot(int(lo) - 1) < slot < ref.slot(int(hi) + 1))
    # (4) the written config names the assembly's own files, and -part1 runs on it
    v1 = drv.readConfigFileToVariables(os.path.join(p1["dir"], "config.txt"))
    assert v1["resolution"] == r and v1["hicProRawMatrixFile"] == p1["hicProRawMatrixFile"]
    assert v1["hicProScaffSizeFile"] == os.path.join(out, "assembly.sizes")
    assert v1["validPairFile"] == v1["restrictionSiteFile"] == os.devnull
    assert v1["originalFastaFile"] == drv.readConfigFileToVariables(cfg)["assembledFastaFile"]
    capsys.readouterr()
    drv.main(["-part1", "-config", os.path.join(p1["dir"], "config.txt")])
    for key in ("chromosomeGroupFile", "dendrogramOrderFile", "binGroupFile"):
        assert os.path.getsize(v1[key]) > 0, key


def test_cli_with_every_scaffold_its_own_chromosome_is_buildmap(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import assembledMap, buildMap, rebinMap, synth
    for key in ("HICMI_BUILDMAP_PLAIN", "HICMI_LIFTMAP_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS"):
        monkeypatch.delenv(key, raising=False)
    lay = synth.make_layout(160)
    counts, lay = synth.make_raw_counts(lay)
    r = lay.resolution
    work = str(tmp_path)
    paths = synth.write_hicpro(os.path.join(work, "in"), lay, None)
    pair_file = os.path.join(work, "in", "synth.allValidPairs")
    synth.write_valid_pairs(pair_file, lay, counts)
    order = os.path.join(work, "orders.txt")
    with open(order, "w") as fh:
        fh.write(ref.order_file_text([[(s, "+")] for s in range(len(lay.scaffold_names))], lay.scaffold_names))
    cfg = synth.write_config(os.path.join(work, "config.txt"), paths, os.path.join(work, "out"), os.path.join(work, "plots"),
                             5 * r, extra={"validPairFile": pair_file})
    a_out, b_out = os.path.join(work, "assembled"), os.path.join(work, "build")
    half = r * 3 // 2
    assembledMap.main(["-config", cfg, "-resolution", "%d,%d" % (r, half), "-order", order, "-out", a_out, "-noBalance"])
    buildMap.main(["-config", cfg, "-resolution", "%d,%d" % (r, half), "-out", b_out, "-noBalance"])
    for res in (r, half):
        a = rebinMap.output_paths(a_out, res, prefix="assembled")["hicProRawMatrixFile"]
        b = rebinMap.output_paths(b_out, res, prefix="build")["hicProRawMatrixFile"]
        assert os.path.getsize(a) > 1000 and _read(a) == _read(b)
