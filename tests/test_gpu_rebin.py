"""Rebinning on the device (hicmi_rebin) against tests/rebin_reference.py: the default kernel and the
HICMI_REBIN_PLAIN=1 kernel, byte for byte on integer counts; the refusals; a
non-integer map against ``math.fsum`` within the worst-case bound of a non-negative sum, (w_I w_J - 1) 2^-53 relative; and
rebinMap -factor 2 followed by -part1 -part2 against -part0 -part1 -part2 on a map the reference rebinned."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ice_reference as ice_ref
import rebin_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -5
FORMS = {"default": {}, "plain": {"HICMI_REBIN_PLAIN": "1"}}


@functools.lru_cache(maxsize=None)
def _case(n):
    counts, lay = ref.make_case(n)
    counts.setflags(write=False)
    return counts, lay


@functools.lru_cache(maxsize=None)
def _reference(n, k):
    counts, lay = _case(n)
    g = ref.group_starts(lay.scaffold_of_bin, k)
    R = ref.reference_rebin(counts, g)
    for a in (g, R):
        a.setflags(write=False)
    return g, R


def _set_form(monkeypatch, form):
    monkeypatch.delenv("HICMI_REBIN_PLAIN", raising=False)
    for key, value in FORMS[form].items():
        monkeypatch.setenv(key, value)


def _device(counts, group_start):
    """(R, both row sums the context holds after the call)."""
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        ctx.set_contacts(counts)
        ctx.rebin(group_start)
        assert ctx.n == len(group_start) - 1
        return ctx.contacts_host(), ctx.row_sums()


@pytest.mark.parametrize("form", ["default", "plain"])
@pytest.mark.parametrize("n,k", ref.CASES)
def test_device_matches_the_reference_bit_for_bit(n, k, form, monkeypatch):
    counts, _lay = _case(n)
    g, Rr = _reference(n, k)
    _set_form(monkeypatch, form)
    R, (np_sum, seq_sum) = _device(counts, g)
    assert R.shape == Rr.shape
    assert R.tobytes() == np.ascontiguousarray(Rr).tobytes()
    # the row sums the context holds are those of the result (integer counts: every order is exact)
    assert np.array_equal(np_sum, Rr.sum(axis=1)) and np.array_equal(seq_sum, Rr.sum(axis=1))


def _alternating(n_pairs):
    """Widths 1, 64, 1, 64, ...: group_start and n."""
    g = np.concatenate([[0], np.cumsum(np.tile([1, 64], n_pairs))])
    return g, int(g[-1])


@pytest.mark.parametrize("form", ["default", "plain"])
@pytest.mark.parametrize("shape", ["ones", "one_group", "alternating"])
def test_hand_made_groups(shape, form, monkeypatch):
    if shape == "ones":
        n = 65
        g = np.arange(n + 1)
    elif shape == "one_group":
        n = 64
        g = np.array([0, 64])
    else:
        g, n = _alternating(33)                                          # 2145 bins: groups across two chunk borders
        assert n == 2145
    rng = np.random.default_rng(n)
    c = np.triu(rng.integers(0, 1000, (n, n)).astype(np.float64))
    c = c + np.triu(c, 1).T
    _set_form(monkeypatch, form)
    R, _sums = _device(c, g)
    if shape == "ones":
        assert R.tobytes() == c.tobytes()                                # all widths 1: the input itself
    elif shape == "one_group":
        assert R.shape == (1, 1) and R[0, 0] == np.triu(c).sum()
    assert R.tobytes() == ref.reference_rebin(c, g).tobytes()


def test_refusals_leave_the_context_usable():
    from hic_genome_assembler_amd import _lib
    counts, lay = _case(65)
    g, Rr = _reference(65, 3)

    def refused(ctx, group_start, code):
        with pytest.raises(_lib.HicmiError) as exc:
            ctx.rebin(group_start)
        assert "error %d:" % code in str(exc.value)

    with _lib.Context(0) as ctx:
        refused(ctx, g, EINVAL)                                          # no matrix set
        ctx.set_contacts(counts)
        refused(ctx, [0, 65], EUNSUPPORTED)                              # one group of 65
        refused(ctx, [1, 30, 65], EINVAL)                                # does not start at 0
        refused(ctx, [0, 30, 64], EINVAL)                                # does not end at n
        refused(ctx, [0, 30, 66], EINVAL)
        refused(ctx, [0, 30, 30, 65], EINVAL)                            # not strictly ascending
        refused(ctx, [0, 40, 30, 65], EINVAL)
        refused(ctx, list(range(66)) + [65], EINVAL)                     # m > n
        with pytest.raises(ValueError):
            ctx.rebin([0])
        assert ctx.n == 65 and ctx.contacts_host().tobytes() == counts.tobytes()
        ctx.rebin(g)
        assert ctx.contacts_host().tobytes() == Rr.tobytes()
        refused(ctx, g, EINVAL)                                          # the matrix is the coarse one now: g ends at 65
        ctx.rebin([0, len(g) - 1])                                       # ... and can be rebinned again
        assert ctx.contacts_host()[0, 0] == np.triu(counts).sum()


@pytest.mark.parametrize("ld,shift", [(65, 0), (68, 0), (66, 1)])
def test_adopted_source_is_read_and_left_untouched(ld, shift, monkeypatch):
    """Odd and even leading dimension, and an even one on a base that is not 16-byte aligned: both load forms."""
    import torch
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    counts, _lay = _case(65)
    g, Rr = _reference(65, 3)
    store = torch.full((65 * ld + 2,), 7.0, dtype=torch.float64, device="cuda:0")   # the padding is never read
    t = store[shift:shift + 65 * ld].view(65, ld)
    assert t.data_ptr() % 16 == 8 * shift
    t[:, :65] = torch.tensor(np.array(counts), device="cuda:0")
    before = t.clone()
    with _lib.Context(0) as ctx:
        ctx.set_contacts_device(t.data_ptr(), 65, ld, keepalive=t)
        ctx.rebin(g)
        assert ctx.contacts_host().tobytes() == Rr.tobytes()
        assert np.array_equal(ctx.row_sums()[0], Rr.sum(axis=1))
        torch.cuda.synchronize()
        assert torch.equal(t, before)
        ctx.ice_balance(None, 3, 0.1)                                    # the result is the context's own: ICE may rewrite it
        torch.cuda.synchronize()
        assert torch.equal(t, before)


@pytest.mark.parametrize("form", ["default", "plain"])
def test_non_integer_input_is_symmetric_reproducible_and_within_the_bound(form, monkeypatch):
    real, lay = ref.make_real_case(257)
    g = ref.group_starts(lay.scaffold_of_bin, 5)
    exact, terms = _exact_257()
    _set_form(monkeypatch, form)
    R, _sums = _device(real, g)
    again, _sums = _device(real, g)
    assert R.tobytes() == again.tobytes()
    assert np.array_equal(R, R.T)
    rel = np.abs(R - exact) / exact
    bound = (terms - 1) * 2.0 ** -53
    print("%s: largest relative error %.3e, largest share of the bound %.3f" % (
        form, rel.max(), (rel[terms > 1] / bound[terms > 1]).max()))
    assert (rel <= bound).all()
    # both kernels keep the one order: the same bits
    _set_form(monkeypatch, "default")
    assert _device(real, g)[0].tobytes() == R.tobytes()


@functools.lru_cache(maxsize=None)
def _exact_257():
    real, lay = ref.make_real_case(257)
    return ref.exact_rebin(real, ref.group_starts(lay.scaffold_of_bin, 5))


# ---- end to end: rebinMap -factor 2, then -part1 -part2 ------------------------------------------------------------------
E2E_FILES = ["dendrogramOrder.txt", "binGroups.txt", "assessment.txt", "chromosomeGroups.txt", "chromosomeOrders.txt",
             "plotOrder.txt"]


def _config(work, paths, resolution, raw):
    from hic_genome_assembler_amd import synth
    return synth.write_config(os.path.join(work, "config.txt"), paths, os.path.join(work, "out"), os.path.join(work, "plots"),
                              resolution, min_size=5, modularity=0.0, psig=0.05, n_scaffolds=6, scan_scaffolds=5,
                              extra={"hicProRawMatrixFile": raw, "iceMinScaffoldSize": 10000})


def _texts(out_dir, bias_file, matrix_file):
    out = {k: open(os.path.join(out_dir, k)).read() for k in E2E_FILES}
    out["biases"] = open(bias_file).read()
    out["matrix"] = open(matrix_file).read()
    return out


def test_rebinned_map_runs_through_part1_and_part2(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import rebinMap, synth
    from hic_genome_assembler_amd import run_hicAssembler as drv
    monkeypatch.setenv("HICMI_LOUVAIN_SEED", "0")
    for key in ("HICMI_ICE_INPLACE", "HICMI_ICE_REPARSE", "HICMI_REBIN_PLAIN"):
        monkeypatch.delenv(key, raising=False)
    lay = synth.make_layout(800, seed=7, n_chrom=3, mean_scaffold_bins=9.0)
    counts, lay = synth.make_raw_counts(lay, seed=7, dead_bins=(123,), short_scaffolds=2, short_size_bp=5000)
    # the coarse map by the reference, and what ICE does on it: the stop decision cannot hinge on rounding
    rows, g = ref.coarse_bed(lay, 2)
    coarse = ref.reference_rebin(counts, g)
    assert len(rows) == 423
    sizes = dict(zip(lay.scaffold_names, lay.scaffold_sizes_bp.tolist()))
    short = np.array([sizes[r[0]] < 10000 for r in rows])
    mask_r, n_a, n_b, n_c = ice_ref.ice_mask(coarse, short)
    _X, _b, iters_r, _d, deltas = ice_ref.ice_balance(coarse, mask_r, 100, 0.1)
    assert iters_r == 6 and ice_ref.stop_margin(deltas, 0.1) >= 1e-6
    # (1) the product: the fine files, rebinMap -factor 2, then -part1 -part2 in a child process on its config
    fine = str(tmp_path / "fine")
    os.makedirs(fine)
    paths = synth.write_hicpro(os.path.join(fine, "in"), lay, None, raw_counts=counts)
    cfg = _config(fine, paths, lay.resolution, paths["hicProRawMatrixFile"])
    out = str(tmp_path / "rebin")
    rebinMap.main(["-config", cfg, "-factor", "2", "-out", out])
    said = capsys.readouterr().out
    assert "REBIN: factor 2, resolution 200000, bins 423 " in said
    assert "masked %d (scaffold size %d, no counts %d, low counts %d), iterations 6" % (mask_r.sum(), n_a, n_b, n_c) in said
    d = os.path.join(out, "res200000")
    new_cfg = os.path.join(d, "config.txt")
    v = drv.readConfigFileToVariables(new_cfg)
    assert v["resolution"] == 200000 and os.path.isdir(v["saveFilesDirectory"]) and os.path.isdir(v["savePlotsDirectory"])
    with open(os.path.join(out, "rebin_summary.tsv")) as fh:
        summary = [ln.split("\t") for ln in fh.read().splitlines()]
    assert summary[0][0] == "#factor" and len(summary) == 2 and len(summary[1]) == len(summary[0]) == 11
    n_scaf = len(lay.scaffold_names)
    one_bin = int((np.bincount(lay.scaffold_of_bin) <= 2).sum())
    assert summary[1][:8] == ["2", "200000", "423", str(n_scaf), str(one_bin), str(n_a), str(n_b), str(n_c)]
    assert summary[1][8] == "6" and float(summary[1][10]) == np.triu(counts).sum()
    with open(v["hicProBiasFile"]) as fh:
        assert fh.read().count("\n") == 423                              # one line per coarse bed line
    res = subprocess.run([sys.executable, os.path.join(ROOT, "run_hicAssembler.py"), "-part1", "-part2", "-config", new_cfg],
                         env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    got = _texts(v["saveFilesDirectory"], v["hicProBiasFile"], v["hicProMatrixFile"])
    # (2) -part0 -part1 -part2 on a bed file and a raw map written here from the reference's coarse map
    work = str(tmp_path / "coarse")
    os.makedirs(os.path.join(work, "in"))
    cpaths = {"hicProBedFile": os.path.join(work, "in", "c_abs.bed"), "hicProBiasFile": os.path.join(work, "in", "c_iced.matrix.biases"),
              "hicProMatrixFile": os.path.join(work, "in", "c_iced.matrix"), "hicProScaffSizeFile": paths["hicProScaffSizeFile"]}
    raw = os.path.join(work, "in", "c.matrix")
    with open(cpaths["hicProBedFile"], "w") as fh:
        fh.write("".join("%s\t%d\t%d\t%d\n" % r for r in rows))
    with open(raw, "w") as fh:
        for i in range(len(rows)):
            fh.write("".join("%d\t%d\t%d\n" % (i + 1, i + j + 1, coarse[i, i + j]) for j in np.flatnonzero(coarse[i, i:])))
    with open(v["hicProBedFile"]) as a, open(cpaths["hicProBedFile"]) as b:
        assert a.read() == b.read()
    ccfg = _config(work, cpaths, 200000, raw)
    drv.main(["-part0", "-part1", "-part2", "-config", ccfg])
    assert "ICE: bins 423, masked" in capsys.readouterr().out
    want = _texts(os.path.join(work, "out"), cpaths["hicProBiasFile"], cpaths["hicProMatrixFile"])
    assert want["chromosomeOrders.txt"].count("\n") > 20 and want["chromosomeGroups.txt"].count("\n") >= 3
    for key in want:
        assert got[key] == want[key], key + " differs"
