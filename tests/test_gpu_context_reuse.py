"""One context over maps of changing size: every buffer group of the context (csrc/devbuf.h) regrows once
(192 -> 320 bins) and then meets "the capacity suffices but the leading dimension differs" (320 -> 192: ldr and ldw 320
against 192).  Every array the reused context returns must equal, bit for bit, what a fresh context returns for the same
map.  Then the context is closed and another is opened and run: tear-down left the device usable.  (Nothing is said about
free memory: on a shared card that figure moves with other people's work.)

The same is asked of every stage family of tests/reuse_cases.py: its three cases on one context give the bytes of three
fresh contexts, family by family and with the families interleaved, so that no family reads what it or another one left in
a buffer.  Fresh contexts are run twice and compared first: bit equality needs run-to-run reproducibility."""
import numpy as np
import pytest

import reuse_cases as rc
from hic_genome_assembler_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (192, 320, 192)                 # the third map is another map than the first: nothing stale may answer for it


@pytest.fixture(scope="module")
def maps():
    out = []
    for k, n in enumerate(SIZES):
        layout = synth.make_layout(n, seed=11 + k)
        out.append((layout, synth.dense_contacts(layout, seed=11 + k)))
    return out


def _selection(layout):
    """Part 2 on the bins of the planted chromosomes 0 .. 3 (half the map): the selection and its scaffold ranges."""
    sel = np.flatnonzero(layout.chrom_of_bin < 4).astype(np.int32)
    scaf = layout.scaffold_of_bin[sel]
    starts = np.flatnonzero(np.r_[True, scaf[1:] != scaf[:-1]]).astype(np.int32)
    lens = np.diff(np.r_[starts, len(sel)]).astype(np.int32)
    return sel, starts, lens


def _run(ctx, layout, c):
    """row_sums, upgma, rank_matrix, the two cut scans and Part 2's select / layout / arrangement / support: every
    returned array, by name."""
    n = len(c)
    got = {}
    ctx.set_contacts(c)
    got["np_sum"], got["seq_sum"] = ctx.row_sums()
    got["leaves"], got["Z"] = ctx.upgma()
    ctx.rank_matrix(got["leaves"])
    got["presort"] = np.array(ctx.presort_state())
    got["rank"], got["rank_inverse"] = ctx.rank_rows(), ctx.rank_rows(inverse=True)
    cuts, m_log = ctx.first_pass_cuts(5, int(n - n * .05), .05)
    kept, warned = ctx.filter_cuts(cuts, .05)
    got["cuts"], got["m_log"] = np.array(cuts), np.array(m_log).reshape(-1, 2)
    got["kept"], got["warned"] = np.array(kept), np.array([warned])
    sel, starts, lens = _selection(layout)
    ctx.p2_select(sel)
    ctx.p2_layout(starts, lens)
    ids = np.arange(len(starts), dtype=np.int32)
    rev = (ids % 3 == 1).astype(np.uint8)
    ctx.p2_set_arrangement(ids, rev)
    total = ctx.p2_arrangement_total()
    got["total"] = np.array([total])
    got["support"], got["support_best"] = ctx.p2_support(ids, rev, total)
    return got


def _same(got, want, what):
    assert sorted(got) == sorted(want)
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key)
        assert a.tobytes() == b.tobytes(), "%s: %s differs from a fresh context's" % (what, key)


def test_one_context_over_maps_of_changing_size(maps, monkeypatch):
    from hic_genome_assembler_amd import _lib
    for var in ("HICMI_NO_PRESORT", "HICMI_SORT_RADIX", "HICMI_SORT_LDS", "HICMI_PRESORT_TIES", "HICMI_HOST_SCANS"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("HICMI_PRESORT_FROM", "64")          # the pre-sort buffers are built at these sizes
    fresh = []
    for layout, c in maps:
        with _lib.Context(0) as ctx:
            fresh.append(_run(ctx, layout, c))
    for want, (layout, c) in zip(fresh, maps):
        # the test exercises what it says: the pre-sort ran, cuts were found, Part 2 had scaffolds to place
        assert want["presort"][0] == 1 and len(want["cuts"]) >= 3 and want["support"].shape[0] >= 4
        assert len(want["Z"]) == len(c) - 1 and want["total"][0] > 0
    assert fresh[1]["support"].shape[0] > fresh[0]["support"].shape[0]       # the layout tables regrow too
    with _lib.Context(0) as ctx:
        for k, (layout, c) in enumerate(maps):
            _same(_run(ctx, layout, c), fresh[k], "map %d (%d bins) on the reused context" % (k, len(c)))
    # the reused context is closed: a second one opens and runs on the same device
    with _lib.Context(0) as ctx:
        _same(_run(ctx, *maps[1]), fresh[1], "a context opened after the tear-down")


# ---- every stage family -------------------------------------------------------------------------------------------------------
FORMS = [(family, "default") for family in rc.FAMILIES] + [(family, "plain") for family in rc.PLAIN_FORMS]
_fresh_cache = {}


def _set_form(monkeypatch, family, form):
    rc.default_forms(monkeypatch)
    if form != "default":
        for key, value in rc.PLAIN_FORMS[family].items():
            monkeypatch.setenv(key, value)


def _fresh(family, form):
    """The three cases of a family, each on a context of its own, run twice: the second run must repeat the first.  (The
    one output that is the race's by design, the order of a plain pair store, is compared in rc.canonical's form.)"""
    from hic_genome_assembler_amd import _lib
    if (family, form) not in _fresh_cache:
        runs = []
        for _repeat in range(2):
            runs.append([])
            for case in rc.cases_of(family):
                with _lib.Context(0) as ctx:
                    runs[-1].append(rc.canonical(family, form, rc.FAMILIES[family](ctx, case)))
        for k, (first, second) in enumerate(zip(*runs)):
            _same(second, first, "%s, case %d, a second fresh context" % (family, k))
        _fresh_cache[family, form] = runs[0]
    return _fresh_cache[family, form]


def _differ(a, b):
    return any(np.asarray(a[key]).shape != np.asarray(b[key]).shape or np.asarray(a[key]).tobytes() != np.asarray(b[key]).tobytes()
               for key in a if key != "sizes")


def _exercises_what_it_says(family, fresh):
    small, large = (0, 1) if family in rc.MATRIX_FAMILIES else (1, 2)
    # a later case needs more of every size the family allocates by ...
    assert (fresh[large]["sizes"] > fresh[small]["sizes"]).all(), (family, fresh[small]["sizes"], fresh[large]["sizes"])
    if family in rc.PAIR_FAMILIES:                           # ... and the pair families shrink first: case 1 needs less than case 0
        assert (fresh[1]["sizes"] < fresh[0]["sizes"]).all() and (fresh[2]["sizes"] > fresh[0]["sizes"]).all(), family
    # ... and the third case is not the first again: something stale would be noticed
    assert _differ(fresh[0], fresh[2]), family
    if family == "part1":
        # the pre-sort ran and was used (dRankS, d_ident, d_ties, d_tie_bits), on the map in whole counts with rows of equal
        # similarities to sort again (d_row_list); cuts were found
        for got in fresh:
            assert got["presort"][0] == 1 and got["tied_presort"][0] == 1 and got["tied_presort"][1] > 0 and len(got["cuts"]) >= 3
    if family in ("p2_tables", "p2_search"):
        assert all(got["sizes"][2] >= 10 for got in fresh)           # scaffolds to place, windows of 7 among them


@pytest.mark.parametrize("family,form", FORMS, ids=["%s-%s" % f for f in FORMS])
def test_family_on_a_reused_context(family, form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, family, form)
    fresh = _fresh(family, form)
    _exercises_what_it_says(family, fresh)
    with _lib.Context(0) as ctx:
        for k, case in enumerate(rc.cases_of(family)):
            got = rc.canonical(family, form, rc.FAMILIES[family](ctx, case))
            _same(got, fresh[k], "%s, case %d on the reused context" % (family, k))


def test_families_interleaved_on_one_context(monkeypatch):
    """Case 0 of every family, case 1 of every family in reverse order, case 2 in the first order, on one context: the
    Part 2 families, the plots and the scans share scratch (d_scores, d_T, d_partial, d_tmp, d_ins_partial and the pinned
    staging), and only interleaving shows a family that reads what another one left there.  The pair families do the same
    on a second context that holds a pair store all the while: the store is loaded before the round's other families run
    and read, by pairs_fetch and by every resident stage, after them."""
    from hic_genome_assembler_amd import _lib
    rc.default_forms(monkeypatch)
    fresh = {family: _fresh(family, "default") for family in rc.FAMILIES}
    matrix, pair = list(rc.MATRIX_FAMILIES), [f for f in rc.PAIR_FAMILIES if f not in ("pairs_store", "resident")]
    with _lib.Context(0) as ctx:
        for k, order in enumerate((matrix, matrix[::-1], matrix)):
            for family in order:
                _same(rc.FAMILIES[family](ctx, rc.matrix_cases()[k]), fresh[family][k], "%s, case %d, interleaved" % (family, k))
    with _lib.Context(0) as ctx:
        for k, order in enumerate((pair, pair[::-1], pair)):
            case = rc.pair_cases()[k]
            rc.load_store(ctx, case)
            for family in order:
                _same(rc.FAMILIES[family](ctx, case), fresh[family][k], "%s, case %d, interleaved beside a pair store" % (family, k))
            _same(rc.read_store(ctx, case), fresh["pairs_store"][k], "the pair store of case %d after the other families" % k)
            _same(rc.read_resident(ctx, case), fresh["resident"][k], "the resident stages of case %d after the other families" % k)
            ctx.pairs_drop()
