"""Raw maps counted on the device from read pairs (hicmi_map_*, hicmi_build_maps) against
tests/buildmap_reference.py: the HICMI_BUILDMAP_PLAIN=1 kernel (one atomic add per pair), the =0 kernel (equal cells of
a slice brought together in LDS) and whichever of them is the default, byte for byte - the counts are integers, there are no
tolerances; misuse; the one-pass driver at four resolutions against the reference and against hicmi_rebin; and
buildMap's files against iceNormalize's and rebinMap's, then through -part1 -part2."""
import functools
import os

import numpy as np
import pytest

import buildmap_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -5
FORMS = {"default": {}, "plain": {"HICMI_BUILDMAP_PLAIN": "1"}, "combine": {"HICMI_BUILDMAP_PLAIN": "0"}}
R = ref.R
# slices that end inside, on and just past a wave (64), a workgroup (256) and the pairs one workgroup brings together (2048)
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5001]


def _set_form(monkeypatch, form):
    for key in ("HICMI_BUILDMAP_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS"):
        monkeypatch.delenv(key, raising=False)
    for key, value in FORMS[form].items():
        monkeypatch.setenv(key, value)


@functools.lru_cache(maxsize=None)
def _scaffolds():
    names, sizes = ref.odd_scaffolds()
    sizes.setflags(write=False)
    assert ref.first_bins(sizes, R)[1] == 277
    return names, sizes


@functools.lru_cache(maxsize=None)
def _pairs(case):
    """The pairs of a case and the reference map at R, computed once."""
    names, sizes = _scaffolds()
    if case == "one_cell":                                   # 100,000 copies of one pair: the worst contention
        pairs = tuple(np.full(100000, v, dtype=t) for v, t in ((3, np.int32), (69 * R + 1, np.int64), (17, np.int32), (R, np.int64)))
    elif case == "one_row":                                  # 100,000 pairs with one end in one bin
        rng = np.random.default_rng(5)
        sb = rng.integers(0, len(names), 100000).astype(np.int32)
        pb = 1 + np.floor(rng.random(100000) * sizes[sb]).astype(np.int64)
        pairs = (np.full(100000, 38, np.int32), np.full(100000, 12 * R, np.int64), sb, pb)
        swap = rng.random(100000) < 0.5
        pairs = (np.where(swap, pairs[2], pairs[0]), np.where(swap, pairs[3], pairs[1]),
                 np.where(swap, pairs[0], pairs[2]), np.where(swap, pairs[1], pairs[3]))
    else:
        pool = ref.edge_pairs(names, sizes, COUNTS[-1], seed=7)
        pairs = tuple(a[:int(case)] for a in pool)
    want = ref.build(pairs, sizes, R)
    for a in pairs + (want,):
        a.setflags(write=False)
    return pairs, want


def test_the_pool_has_the_cases_the_kernels_must_get_right():
    names, sizes = _scaffolds()
    (sa, pa, sb, pb), want = _pairs(COUNTS[-1])
    first, m = ref.first_bins(sizes, R)
    i, j = first[sa] + (pa - 1) // R, first[sb] + (pb - 1) // R
    assert (i < j).any() and (i > j).any() and (i == j).sum() > 300                    # both mate orders, one bin
    assert (pa == 1).any() and (pa == sizes[sa]).any() and (pb == sizes[sb]).any()
    assert ((pa % R == 0) & (pa < sizes[sa])).any() and ((pa % R == 1) & (pa > 1)).any()   # k r and k r + 1
    assert np.array_equal(want, want.T) and np.triu(want).sum() == COUNTS[-1] and want.max() > 1
    assert _pairs("one_cell")[1].max() == 100000 and np.count_nonzero(_pairs("one_cell")[1]) == 2
    row = _pairs("one_row")[1]
    others = np.arange(m) != first[38] + 11                                              # every pair has an end in that bin
    assert not row[np.ix_(others, others)].any() and np.count_nonzero(row) > m and np.triu(row).sum() == 100000


def _count(sizes, r, parts):
    """(map, pairs returned by finish, both row sums) after one add call per element of ``parts``."""
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        ctx.map_begin(sizes, r)
        for p in parts:
            ctx.map_add_pairs(*p)
        n = ctx.map_finish()
        assert ctx.n == ref.first_bins(sizes, r)[1]
        return ctx.contacts_host(), n, ctx.row_sums()


@pytest.mark.parametrize("form", ["default", "plain", "combine"])
@pytest.mark.parametrize("case", COUNTS + ["one_cell", "one_row"])
def test_add_pairs_matches_the_reference_bit_for_bit(case, form, monkeypatch):
    names, sizes = _scaffolds()
    pairs, want = _pairs(case)
    _set_form(monkeypatch, form)
    got, n, (np_sum, seq_sum) = _count(sizes, R, [pairs])
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert n == len(pairs[0]) == np.triu(got).sum()
    assert np.array_equal(got, got.T)
    assert np.array_equal(np_sum, want.sum(axis=1)) and np.array_equal(seq_sum, want.sum(axis=1))


@pytest.mark.parametrize("form", ["default", "plain", "combine"])
def test_three_calls_equal_one_and_other_resolutions(form, monkeypatch):
    names, sizes = _scaffolds()
    pairs, want = _pairs(COUNTS[-1])
    _set_form(monkeypatch, form)
    cuts = [0, 100, 2500, COUNTS[-1]]
    parts = [tuple(a[cuts[k]:cuts[k + 1]] for a in pairs) for k in range(3)]
    got, n, _sums = _count(sizes, R, parts + [tuple(a[:0] for a in pairs)])
    assert got.tobytes() == want.tobytes() and n == COUNTS[-1]
    for r in (1, 2 * R + 1, 10 ** 7, 2 ** 33):               # one bin per base of a short genome; 64-bit division
        small = (np.array([1, 7, 300], dtype=np.int64) if r == 1 else sizes)
        sub = pairs if r != 1 else (np.array([0, 2, 1, 2], np.int32), np.array([1, 300, 7, 150], np.int64),
                                    np.array([2, 0, 1, 2], np.int32), np.array([1, 1, 7, 150], np.int64))
        got, _n, _sums = _count(small, r, [sub])
        assert got.tobytes() == ref.build(sub, small, r).tobytes()


def test_one_bin_and_a_second_build_replaces_the_first(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    names, sizes = _scaffolds()
    pairs, want = _pairs(257)
    one = (np.zeros(3, np.int32), np.array([1, 5, 3], np.int64), np.zeros(3, np.int32), np.array([5, 5, 1], np.int64))
    with _lib.Context(0) as ctx:
        ctx.map_begin([5], 10)
        ctx.map_add_pairs(*one)
        assert ctx.map_finish() == 3 and ctx.n == 1
        assert ctx.contacts_host().tolist() == [[3.0]] and ctx.row_sums()[0].tolist() == [3.0]
        ctx.map_begin(sizes, R)                                # the 1 x 1 map stays until finish
        assert ctx.contacts_host().tolist() == [[3.0]]
        ctx.map_add_pairs(*pairs)
        ctx.map_begin(sizes, R)                                # a begin gives up the open build: nothing of it is left
        ctx.map_add_pairs(*pairs)
        assert ctx.map_finish() == 257 and ctx.n == 277
        assert ctx.contacts_host().tobytes() == want.tobytes()
        ctx.ice_balance(None, 2, 0.1)                          # the map is the context's own


def test_misuse_leaves_the_matrix_and_a_later_build_right(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    names, sizes = _scaffolds()
    pairs, want = _pairs(257)
    sa, pa, sb, pb = (a.copy() for a in pairs)
    held = np.arange(25, dtype=np.float64).reshape(5, 5)
    held = held + held.T

    def refused(call, code=EINVAL):
        with pytest.raises(_lib.HicmiError) as exc:
            call()
        assert "error %d:" % code in str(exc.value), str(exc.value)

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out

    with _lib.Context(0) as ctx:
        refused(lambda: ctx.map_add_pairs(sa, pa, sb, pb))                     # no begin, no matrix
        refused(ctx.map_finish)
        ctx.set_contacts(held)
        refused(lambda: ctx.map_add_pairs(sa, pa, sb, pb))
        refused(ctx.map_finish)
        refused(lambda: ctx.map_begin(sizes, 0))
        refused(lambda: ctx.map_begin([-1, 5], 10))
        refused(lambda: ctx.map_begin([0, 0], 10))
        refused(lambda: ctx.map_begin([65537 * 10], 10), EUNSUPPORTED)
        refused(ctx.map_finish)                                              # none of them opened a build
        assert ctx.n == 5 and ctx.contacts_host().tobytes() == held.tobytes()
        ctx.map_begin(sizes, R)
        refused(lambda: ctx.map_add_pairs(changed(sa, 200, len(sizes)), pa, sb, pb))
        refused(lambda: ctx.map_add_pairs(sa, pa, changed(sb, 0, -1), pb))
        refused(lambda: ctx.map_add_pairs(sa, changed(pa, 256, 0), sb, pb))
        refused(lambda: ctx.map_add_pairs(sa, pa, sb, changed(pb, 100, sizes[sb[100]] + 1)))
        with pytest.raises(ValueError):
            ctx.map_add_pairs(sa, pa[:5], sb, pb)
        assert ctx.n == 5 and ctx.contacts_host().tobytes() == held.tobytes()
        assert np.array_equal(ctx.row_sums()[0], held.sum(axis=1))
        # nothing of the refused calls was counted: the open build goes on
        ctx.map_add_pairs(sa, pa, sb, pb)
        assert ctx.map_finish() == 257
        assert ctx.contacts_host().tobytes() == want.tobytes()
        refused(ctx.map_finish)                                              # finish closed it
    # a context destroyed between begin and finish
    ctx = _lib.Context(0)
    ctx.map_begin(sizes, R)
    ctx.map_add_pairs(sa, pa, sb, pb)
    ctx.close()


# ---- the driver: one pass, several resolutions -----------------------------------------------------------------------------
RESOLUTIONS = [R, 2 * R, 3 * R, R * 3 // 2]


@functools.lru_cache(maxsize=None)
def _odd_file():
    names, sizes = _scaffolds()
    data = ref.odd_file_bytes(names, sizes, 5000, seed=23)
    pairs, stats, _after = ref.parse_text(data, names, sizes)
    maps = tuple(ref.build(pairs, sizes, r) for r in RESOLUTIONS)
    for a in maps:
        a.setflags(write=False)
    return data, stats, maps


def _write(tmp_path, data):
    path = str(tmp_path / "pairs.allValidPairs")
    with open(path, "wb") as fh:
        fh.write(data)
    return path


@pytest.mark.parametrize("form", ["default", "plain", "combine"])
@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("chunk", ["512", None])
def test_build_maps_at_four_resolutions_in_one_pass(chunk, threads, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib, hostio
    names, sizes = _scaffolds()
    data, stats, maps = _odd_file()
    path = _write(tmp_path, data)
    _set_form(monkeypatch, form)
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    ctxs = [_lib.Context(0) for _r in RESOLUTIONS]
    try:
        got = _lib.build_maps(path, names, sizes, RESOLUTIONS, ctxs, threads=threads)
        assert got[:4] == stats
        assert got[4] == (-(-stats[1] // 512) if chunk else 1) and stats[1] > 4 * 512
        for ctx, want in zip(ctxs, maps):
            assert ctx.n == len(want) and ctx.contacts_host().tobytes() == want.tobytes()
            assert np.array_equal(ctx.row_sums()[0], want.sum(axis=1))
        # the maps at 2 r and 3 r are the map at r rebinned, bit for bit
        fine = hostio.bins_from_sizes((names, sizes), R)
        ptr, n, ld = ctxs[0].contacts_device()
        for k in (2, 3):
            _coarse, group_start = hostio.rebin_bins(fine, k)
            with _lib.Context(0) as other:
                other.set_contacts_device(ptr, n, ld, keepalive=ctxs[0])
                other.rebin(group_start)
                assert other.contacts_host().tobytes() == ctxs[k - 1].contacts_host().tobytes()
    finally:
        for ctx in ctxs:
            ctx.close()


@pytest.mark.parametrize("chunk", ["512", None])
def test_build_maps_error_changes_no_context(chunk, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    data, _stats, maps = _odd_file()
    path = _write(tmp_path, data + b"\nread\tscaffold_4\t12x\t+\tscaffold_4\t5\n")
    _set_form(monkeypatch, "default")
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    held = held + held.T
    with _lib.Context(0) as a, _lib.Context(0) as b:
        a.set_contacts(held)
        with pytest.raises(_lib.HicmiError) as exc:
            _lib.build_maps(path, names, sizes, [R, 2 * R], [a, b])
        assert "error %d:" % EINVAL in str(exc.value) and str(exc.value).endswith("at byte %d" % (len(data) + 1))
        assert a.n == 4 and a.contacts_host().tobytes() == held.tobytes()
        with pytest.raises(_lib.HicmiError):
            b.contacts_device()                                              # it had no matrix and has none
        for call in (a.map_finish, b.map_finish):                            # and no build is left open
            with pytest.raises(_lib.HicmiError):
                call()
        with pytest.raises(_lib.HicmiError) as exc:                          # refused before the file is opened
            _lib.build_maps(str(tmp_path / "missing"), names, np.array(sizes) * 10, [R, 1], [a, b])
        assert "error %d:" % EUNSUPPORTED in str(exc.value) and "resolution 1 " in str(exc.value)
        with pytest.raises(_lib.HicmiError):
            _lib.build_maps(path, names, sizes, [R, 2 * R], [a, a])          # one context per resolution
        # the good file afterwards
        good = _write(tmp_path, data)
        _lib.build_maps(good, names, sizes, [R, 2 * R], [a, b])
        assert a.contacts_host().tobytes() == maps[0].tobytes() and b.contacts_host().tobytes() == maps[1].tobytes()


@pytest.mark.parametrize("setting", ["0", str(2 ** 28 + 1)])
def test_a_chunk_setting_out_of_range_is_refused_by_every_file_call(setting, tmp_path, monkeypatch):
    """HICMI_BUILDMAP_CHUNK_PAIRS is read in one place for all seven passes over a pair file: each of them refuses a value
    outside 1 .. 2^28 by name, before it opens a build or a store, and the context's matrix stays what it was."""
    import liftmap_reference as lref
    import split_reference as sref
    from hic_genome_assembler_amd import _lib
    names, sizes = _scaffolds()
    path = _write(tmp_path, _odd_file()[0])
    lift = lref.layout([[(3, "+"), (17, "-")], [(38, "+"), (0, "+")]], sizes, 100, drop_unplaced=True)
    first, start = sref.make_pieces(sizes, {3: [R], 38: [5, 2 * R]})[:2]
    _set_form(monkeypatch, "default")
    monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", setting)
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    held = held + held.T
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held)
        calls = {
            "build_maps": lambda: _lib.build_maps(path, names, sizes, [R], [ctx]),
            "lift_maps": lambda: _lib.lift_maps(path, names, sizes, *lift, [R], [ctx]),
            "split_maps": lambda: _lib.split_maps(path, names, sizes, first, start, [R], [ctx]),
            "span_file": lambda: _lib.span_file(path, names, sizes, *lift, R, 0, 1, [], ctx),
            "ends_file": lambda: _lib.ends_file(path, names, sizes, *lift, R, 1, ctx),
            "anchor_file": lambda: _lib.anchor_file(path, names, sizes, *lift, None, R, ctx),
            "pairs_file": lambda: _lib.pairs_file(path, names, sizes, ctx),
        }
        for name, call in calls.items():
            with pytest.raises(_lib.HicmiError) as exc:
                call()
            assert "error %d:" % EINVAL in str(exc.value) and "HICMI_BUILDMAP_CHUNK_PAIRS = %s " % setting in str(exc.value), name
        assert ctx.n == 4 and ctx.contacts_host().tobytes() == held.tobytes()
        for closing in (ctx.map_finish, lambda: ctx.span_finish(1, []), ctx.ends_finish, ctx.anchor_finish, ctx.pairs_info):
            with pytest.raises(_lib.HicmiError):                                 # nothing was left open
                closing()
        # the same calls with the setting gone, on the same context
        monkeypatch.delenv("HICMI_BUILDMAP_CHUNK_PAIRS")
        assert _lib.pairs_file(path, names, sizes, ctx)[:4] == _odd_file()[1]
        assert _lib.build_maps(path, names, sizes, [R], [ctx])[:4] == _odd_file()[1]
        assert ctx.contacts_host().tobytes() == _odd_file()[2][0].tobytes()


# ---- round trip and drop-in ------------------------------------------------------------------------------------------------
def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("sort", [True, False])
def test_round_trip_and_drop_in(sort, tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import buildMap, hostio, iceNormalize, rebinMap, synth
    from hic_genome_assembler_amd import run_hicAssembler as drv
    monkeypatch.setenv("HICMI_LOUVAIN_SEED", "0")
    for key in ("HICMI_ICE_INPLACE", "HICMI_ICE_REPARSE", "HICMI_REBIN_PLAIN", "HICMI_BUILDMAP_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS"):
        monkeypatch.delenv(key, raising=False)
    monkeypatch.setenv("HICMI_NO_PLOTS", "1")
    lay = synth.make_layout(160)
    counts, lay = synth.make_raw_counts(lay)
    r = lay.resolution
    work = str(tmp_path)
    paths = synth.write_hicpro(os.path.join(work, "in"), lay, None)
    pair_file = os.path.join(work, "in", "synth.allValidPairs")
    n_pairs = synth.write_valid_pairs(pair_file, lay, counts, sort=sort)
    # the config's own resolution is not one of those asked for, and it names no raw map
    cfg = synth.write_config(os.path.join(work, "config.txt"), paths, os.path.join(work, "out"), os.path.join(work, "plots"),
                             5 * r, extra={"validPairFile": pair_file})
    out = os.path.join(work, "build")
    buildMap.main(["-config", cfg, "-resolution", "%d,%d" % (r, 2 * r), "-out", out, "-threads", "3"])
    said = capsys.readouterr().out
    assert "BUILD: lines %d, pairs used %d, unknown scaffold 0, out of range 0, chunks 1" % (n_pairs, n_pairs) in said
    assert "WARNING" not in said
    d1, d2 = os.path.join(out, "res%d" % r), os.path.join(out, "res%d" % (2 * r))
    p1, p2 = rebinMap.output_paths(out, r, prefix="build"), rebinMap.output_paths(out, 2 * r, prefix="build")
    assert p1["hicProRawMatrixFile"] == os.path.join(d1, "build_%d.matrix" % r)
    # (1) the raw map at the layout's resolution is raw_counts, and its bed file is the layout's
    bins = hostio.read_bed_bins(p1["hicProBedFile"])
    assert _read(p1["hicProBedFile"]) == _read(paths["hicProBedFile"])
    assert hostio.read_contact_matrix(p1["hicProRawMatrixFile"], bins).tobytes() == counts.tobytes()
    # (2) iced matrix and biases are what iceNormalize writes from that raw file
    ice_m, ice_b = os.path.join(work, "ice_iced.matrix"), os.path.join(work, "ice_iced.matrix.biases")
    iceNormalize.runPipeline(p1["hicProBedFile"], p1["hicProRawMatrixFile"], paths["hicProScaffSizeFile"], ice_m, ice_b)
    assert _read(p1["hicProMatrixFile"]) == _read(ice_m) and _read(p1["hicProBiasFile"]) == _read(ice_b)
    # (3) the summary
    with open(os.path.join(out, "build_summary.tsv")) as fh:
        summary = [ln.split("\t") for ln in fh.read().splitlines()]
    assert summary[0] == ["#lines=%d" % n_pairs, "used=%d" % n_pairs, "unknown_scaffold=0", "out_of_range=0"]
    assert summary[1][0] == "#resolution" and len(summary) == 4 and len(summary[1]) == len(summary[2]) == len(summary[3]) == 10
    assert summary[2][:2] == [str(r), "160"] and summary[3][0] == str(2 * r)
    assert float(summary[2][9]) == float(summary[3][9]) == n_pairs
    # (4) the directory at 2 r is rebinMap -factor 2 on the first
    v1 = drv.readConfigFileToVariables(os.path.join(d1, "config.txt"))
    assert v1["resolution"] == r and v1["hicProRawMatrixFile"] == p1["hicProRawMatrixFile"] and v1["validPairFile"] == pair_file
    re_out = os.path.join(work, "rebin")
    rebinMap.main(["-config", os.path.join(d1, "config.txt"), "-factor", "2", "-out", re_out])
    q2 = rebinMap.output_paths(re_out, 2 * r)
    for key in ("hicProBedFile", "hicProRawMatrixFile", "hicProMatrixFile", "hicProBiasFile"):
        assert _read(p2[key]) == _read(q2[key]), key + " differs from rebinMap's"
    # (5) -part1 -part2 on the written config
    capsys.readouterr()
    drv.main(["-part1", "-part2", "-config", os.path.join(d1, "config.txt")])
    for key in ("chromosomeGroupFile", "chromosomeOrderFile", "dendrogramOrderFile", "binGroupFile", "plotOrderFile"):
        assert os.path.getsize(v1[key]) > 0, key
