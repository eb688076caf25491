"""The end-link graph on the device (hicmi_links_resident, hicmi_links_fetch) against tests/links_reference.py,
for HICMI_LINKS_PLAIN =1 and =0 on every case and unset on some.  Rows and counters are integers, so every comparison is
exact: there are no tolerances.  The refusal of a table above 2^31 slots needs a store of more than 2^30 pairs and is held
on the host instead (the capacity rule in tests/test_links_cpu.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import ends_reference as eref
import links_reference as ref
import pairs_reference as pref
import test_links_cpu as cpu

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -5
# Both count forms give the same rows by design: these tests hold each to the reference but cannot tell which kernel ran; that
# the switch is read per call is checked from the source in tests/test_links_cpu.py.
FORMS = {"default": {}, "plain": {"HICMI_LINKS_PLAIN": "1"}, "combine": {"HICMI_LINKS_PLAIN": "0"}}
BOTH = ["plain", "combine"]


def _constants():
    from hic_genome_assembler_amd import _lib
    return _lib.LINKS_SLICE, _lib.LINKS_SLOTS


SLICE, SLOTS = _constants()


def _set_form(monkeypatch, form, first_pairs=None):
    for key in ("HICMI_LINKS_PLAIN", "HICMI_PAIRS_PLAIN", "HICMI_PAIRS_FIRST_PAIRS", "HICMI_BUILDMAP_CHUNK_PAIRS"):
        monkeypatch.delenv(key, raising=False)
    for key, value in FORMS[form].items():
        monkeypatch.setenv(key, value)
    if first_pairs is not None:
        monkeypatch.setenv("HICMI_PAIRS_FIRST_PAIRS", str(first_pairs))


def _run(sizes, window, parts, ctx=None):
    from hic_genome_assembler_amd import _lib
    if ctx is None:
        with _lib.Context(0) as own:
            return _run(sizes, window, parts, own)
    ctx.pairs_begin(sizes)
    try:
        for p in parts:
            ctx.pairs_add(*p)
        return ctx.links_resident(sizes, window)
    finally:
        ctx.pairs_drop()


def _want(pairs, sizes, window):
    kept = pref.keep(pairs)
    if len(kept[0]) == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 5), np.uint64), np.zeros(2, np.uint64)
    return ref.rows(kept, sizes, window)


def _same(got, want, n_kept):
    lo, hi, counts, counters = want
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].tolist() == lo.tolist() and got[1].tolist() == hi.tolist()
    assert got[2].dtype == np.uint64 and got[2].shape == counts.shape and got[2].tobytes() == counts.tobytes()
    assert got[3].dtype == np.uint64 and got[3].shape == (2,) and got[3].tolist() == counters.tolist()
    # the invariants: the sum of all counts is the pairs kept, and so is linked plus middle
    assert int(got[2].sum()) == n_kept == int(got[3].sum()) and int(got[2][:, :4].sum()) == int(got[3][0])


def _both_forms(monkeypatch, sizes, window, parts, want, n_kept, forms=BOTH, **env):
    made = []
    for form in forms:
        _set_form(monkeypatch, form, **env)
        made.append(_run(sizes, window, parts))
        _same(made[-1], want, n_kept)
    for other in made[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(made[0], other))     # the forms with each other


@functools.lru_cache(maxsize=None)
def _planted():
    P = eref.planted(seed=7)
    for a in P["pairs"]:
        a.setflags(write=False)
    want = _want(P["pairs"], P["sizes"], eref.PLANTED_WINDOW)
    return P, want, int(pref.mask(P["pairs"]).sum())


def test_planted_pairs(monkeypatch):
    P, want, n_kept = _planted()
    assert n_kept == 17334 and len(want[0]) > 500
    _both_forms(monkeypatch, P["sizes"], eref.PLANTED_WINDOW, [P["pairs"]], want, n_kept, forms=["default", "plain", "combine"])


@pytest.mark.parametrize("window", [1, 5, 10 ** 6])
def test_zone_edges(window, monkeypatch):
    pairs = cpu.random_pairs(cpu.ZONE_SIZES, 2000, window)
    _both_forms(monkeypatch, cpu.ZONE_SIZES, window, [pairs], _want(pairs, cpu.ZONE_SIZES, window), 2000)


@functools.lru_cache(maxsize=None)
def _slice_pool():
    sizes = np.arange(50, 50 + 23, dtype=np.int64)
    return sizes, cpu.random_pairs(sizes, SLICE + 1, 5)


@pytest.mark.parametrize("n", [SLICE - 1, SLICE, SLICE + 1, 255, 256, 257, 1])
def test_slice_and_workgroup_edges(n, monkeypatch):
    sizes, pool = _slice_pool()
    pairs = tuple(a[:n] for a in pool)
    _both_forms(monkeypatch, sizes, 7, [pairs], _want(pairs, sizes, 7), n)


def test_one_key_more_pairs_than_a_slice(monkeypatch):
    # every pair on the key (1, 3, RL): the counts in LDS, one global add per workgroup
    n = 2 * SLICE + 37
    sizes = np.array([10, 10, 10, 10], dtype=np.int64)
    pairs = (np.full(n, 3, np.int32), np.ones(n, np.int64), np.full(n, 1, np.int32), np.full(n, 10, np.int64))
    want = _want(pairs, sizes, 2)
    assert want[0].tolist() == [1] and want[1].tolist() == [3] and want[2].tolist() == [[0, 0, n, 0, 0]] and want[3].tolist() == [n, 0]
    _both_forms(monkeypatch, sizes, 2, [pairs], want, n)


def test_all_keys_distinct_at_the_half_full_bound(monkeypatch):
    # 59 scaffolds have 5 x 1,711 = 8,555 keys; 8,192 of them, one pair each, in a permuted order: four times the slots of the
    # table in LDS, so adds spill to the global table, which 2 x 8,192 = 16,384 slots load to exactly one half
    from hic_genome_assembler_amd import _lib
    n = 4 * SLOTS
    S = 59
    assert n <= 5 * S * (S - 1) // 2 and _lib.links_capacity(n, S) == 2 * n == ref.capacity(n, S)
    sizes = np.full(S, 10, dtype=np.int64)
    lo, hi = np.triu_indices(S, 1)
    lo, hi, combo = np.repeat(lo, 5), np.repeat(hi, 5), np.tile(np.arange(5), len(lo))
    keep = np.random.default_rng(3).permutation(len(lo))[:n]
    lo, hi, combo = lo[keep], hi[keep], combo[keep]
    # window 2: base 1 is left, base 10 right, base 5 in the middle
    p_lo = np.where(combo == ref.OTHER, 5, np.where(combo // 2 == 0, 1, 10))
    p_hi = np.where(combo == ref.OTHER, 1, np.where(combo % 2 == 0, 1, 10))
    pairs = (hi.astype(np.int32), p_hi.astype(np.int64), lo.astype(np.int32), p_lo.astype(np.int64))
    want = _want(pairs, sizes, 2)
    assert int((want[2] > 0).sum()) == n and int(want[2].max()) == 1
    _both_forms(monkeypatch, sizes, 2, [pairs], want, n)


def test_an_empty_store_and_a_store_of_intra_pairs_give_no_rows(monkeypatch):
    sizes = np.array([10, 10, 10], dtype=np.int64)
    none = cpu._pairs([])
    intra = cpu._pairs([(1, 2, 1, 9)] * 5)
    for parts in ([], [none], [intra]):
        _both_forms(monkeypatch, sizes, 2, parts, _want(none, sizes, 2), 0)


def test_a_grown_store_a_reordered_store_and_a_second_call(monkeypatch):
    from hic_genome_assembler_amd import _lib
    pairs = cpu.random_pairs(cpu.ZONE_SIZES, 2000, 5)
    want = _want(pairs, cpu.ZONE_SIZES, 5)
    parts = [tuple(a[k:k + 300] for a in pairs) for k in range(0, 2000, 300)]
    _both_forms(monkeypatch, cpu.ZONE_SIZES, 5, parts, want, 2000, first_pairs=256)          # several growths
    sa, pa, sb, pb = pairs
    order = np.random.default_rng(9).permutation(2000)
    _both_forms(monkeypatch, cpu.ZONE_SIZES, 5, [(sb[order], pb[order], sa[order], pa[order])], want, 2000)
    for store in ("0", "1"):                                                                 # either store order
        _set_form(monkeypatch, "combine")
        monkeypatch.setenv("HICMI_PAIRS_PLAIN", store)
        _same(_run(cpu.ZONE_SIZES, 5, [pairs]), want, 2000)
    # the rows of a second call at another window replace the first; pairs added afterwards make them stale
    _set_form(monkeypatch, "default")
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(cpu.ZONE_SIZES)
        ctx.pairs_add(*pairs)
        _same(ctx.links_resident(cpu.ZONE_SIZES, 5), want, 2000)
        _same(ctx.links_resident(cpu.ZONE_SIZES, 1), _want(pairs, cpu.ZONE_SIZES, 1), 2000)
        ctx.pairs_add(*(a[:10] for a in pairs))
        rc = ctx._lib.hicmi_links_fetch(ctx._h, None, None, None)
        assert rc == EINVAL and "hicmi_links_fetch before hicmi_links_resident" in _lib.load().hicmi_last_error().decode()
        twice = tuple(np.concatenate([a, a[:10]]) for a in pairs)
        _same(ctx.links_resident(cpu.ZONE_SIZES, 5), _want(twice, cpu.ZONE_SIZES, 5), 2010)
        ctx.pairs_drop()
        assert ctx._lib.hicmi_links_fetch(ctx._h, None, None, None) == EINVAL


# ---- refusals: every one leaves marked output buffers untouched -------------------------------------------------------------------------
def _raw(ctx, sizes, window, n_scaf=None, null=None):
    from hic_genome_assembler_amd import _lib
    size = np.ascontiguousarray(sizes, dtype=np.int64)
    counters = np.full(2, 0xABAB, np.uint64)
    n_rows = ctypes.c_int64(-7)
    outs = [ctypes.byref(n_rows), _lib._ptr(counters)]
    if null is not None:
        outs[null] = None
    rc = ctx._lib.hicmi_links_resident(ctx._h, _lib._ptr(size), len(size) if n_scaf is None else n_scaf, int(window), *outs)
    return rc, n_rows.value, counters.tolist(), _lib.load().hicmi_last_error().decode("utf-8", "replace")


def _unwritten(got):
    return got[1] == -7 and got[2] == [0xABAB, 0xABAB]


def test_refusals_leave_the_outputs_and_the_rows_as_they_were(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    sizes = cpu.ZONE_SIZES
    pairs = cpu.random_pairs(sizes, 500, 2)
    want = _want(pairs, sizes, 5)
    marks = (np.full(3, -9, np.int32), np.full(3, -9, np.int32), np.full(15, 77, np.uint64))

    def fetch_refused(ctx):
        rc = ctx._lib.hicmi_links_fetch(ctx._h, *(_lib._ptr(m) for m in marks))
        return rc == EINVAL and "hicmi_links_fetch before hicmi_links_resident" in _lib.load().hicmi_last_error().decode() \
            and marks[0].tolist() == [-9] * 3 and marks[1].tolist() == [-9] * 3 and marks[2].tolist() == [77] * 15

    with _lib.Context(0) as ctx:
        got = _raw(ctx, sizes, 5)
        assert got[0] == EINVAL and "hicmi_links_resident without a pair store" in got[3] and _unwritten(got)
        assert fetch_refused(ctx)
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        assert fetch_refused(ctx)                                                     # a store, but no count yet
        other = sizes.copy()
        other[3] += 1
        for got, code, word in ((_raw(ctx, other, 5), EINVAL, "sizes"),
                                (_raw(ctx, sizes[:-1], 5), EINVAL, "sizes"),
                                (_raw(ctx, sizes, 0), EINVAL, "window 0 is below 1"),
                                (_raw(ctx, sizes, -5), EINVAL, "window"),
                                (_raw(ctx, sizes, 5, n_scaf=(1 << 30) + 1), EUNSUPPORTED, "%d scaffolds" % ((1 << 30) + 1)),
                                (_raw(ctx, sizes, 5, null=0), EINVAL, "bad arguments"),
                                (_raw(ctx, sizes, 5, null=1), EINVAL, "bad arguments")):
            assert got[0] == code and word in got[3] and _unwritten(got), got
        assert fetch_refused(ctx)
        # a count, then refusals: the rows of the count stay
        _same(ctx.links_resident(sizes, 5), want, 500)
        assert _raw(ctx, sizes, 0)[0] == EINVAL and _raw(ctx, other, 5)[0] == EINVAL
        lo, hi, counts = np.zeros(len(want[0]), np.int32), np.zeros(len(want[0]), np.int32), np.zeros((len(want[0]), 5), np.uint64)
        assert ctx._lib.hicmi_links_fetch(ctx._h, _lib._ptr(lo), _lib._ptr(hi), _lib._ptr(counts)) == 0
        assert lo.tolist() == want[0].tolist() and hi.tolist() == want[1].tolist() and counts.tobytes() == want[2].tobytes()
        ctx.pairs_drop()
        assert fetch_refused(ctx)                                                     # the rows went with the store
        with pytest.raises(_lib.HicmiError) as exc:
            ctx.links_resident(sizes, 5)
        assert "error %d:" % EINVAL in str(exc.value) and "without a pair store" in str(exc.value)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_cli_on_the_planted_pair_file_and_placeunplaced_on_its_paths(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import placeUnplaced, scaffoldLinks
    _set_form(monkeypatch, "default")
    P, cfg, order, _save = cpu.planted_files(tmp_path)
    files = ("links.tsv", "ends.tsv", "paths.order", "links_summary.tsv", "junctions.tsv")
    made = {}
    for where, context in (("device", None), ("stand_in", ref.StandInContext())):
        out = str(tmp_path / where)
        _stats, joins, paths = scaffoldLinks.main(["-config", cfg, "-window", "5000", "-order", order, "-out", out, "-threads", "3"],
                                                  context=context)
        assert len(joins) == 32 and len(paths) == 8
        made[where] = [cpu._read(os.path.join(out, fn)) for fn in files]
    assert made["device"] == made["stand_in"]
    assert capsys.readouterr().out.count("LINKS: scaffolds 40, pairs kept 17334, rows %d, joins 32, paths 8\n" % len(_planted()[1][0])) == 2
    # the paths are an order file placeUnplaced runs on: every scaffold lies in a path, so it has nothing to place
    report = str(tmp_path / "unplaced.txt")
    placeUnplaced.main(["-config", cfg, "-order", os.path.join(str(tmp_path / "device"), "paths.order"), "-window", "5000", "-out", report])
    assert os.path.isfile(report)
