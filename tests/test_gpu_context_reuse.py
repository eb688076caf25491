"""One context over maps of changing size: every buffer group of the context (csrc/devbuf.h) regrows once
(192 -> 320 bins) and then meets "the capacity suffices but the leading dimension differs" (320 -> 192: ldr and ldw 320
against 192).  Every array the reused context returns must equal, bit for bit, what a fresh context returns for the same
map.  Then the context is closed and another is opened and run: tear-down left the device usable.  (Nothing is said about
free memory: on a shared card that figure moves with other people's work.)"""
import numpy as np
import pytest

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
