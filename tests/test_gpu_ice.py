"""Part 0 on the device (hicmi_ice_mask_rows, hicmi_ice_balance) against tests/ice_reference.py, the
literal NumPy loop: both paths (the read-only u formulation and HICMI_ICE_INPLACE=1), and -part0 handing its matrix to
Part 1 in HBM against a run that reads the written files.

Bound: 1e-10 relative on values and biases (1e-10 max|X| where the reference value is 0), the bound the project holds a
re-associated form to against a literal evaluation.  The stop decision cannot hinge on rounding: on
the reference alone, every sum |bias_prev - bias| the stop test looks at is at least 1e-6 (relative) away from eps."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ice_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-10
ESTATE = -4


@functools.lru_cache(maxsize=None)
def _case(n):
    counts, lay, short = ref.make_case(n)
    mask, n_a, n_b, n_c = ref.ice_mask(counts, short)
    for a in (counts, mask):
        a.setflags(write=False)
    return counts, lay, short, mask, (n_a, n_b, n_c)


@functools.lru_cache(maxsize=None)
def _reference(n, eps, max_iter):
    counts, _lay, _short, mask, _k = _case(n)
    X, bias, iters, delta, deltas = ref.ice_balance(counts, mask, max_iter, eps)
    X.setflags(write=False)
    bias.setflags(write=False)
    return X, bias, iters, delta, tuple(deltas)


def _device(n, eps, max_iter):
    """The product's own sequence on the device: returns (mask, counts by rule, X, bias, iterations, delta)."""
    from hic_genome_assembler_amd import _lib, iceNormalize
    counts, _lay, short, _mask, _k = _case(n)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(counts)
        mask, by_rule, bias, iters, delta = iceNormalize.balanceResident(ctx, short, 0.02, max_iter, eps)
        X = ctx.contacts_host()
    return mask, by_rule, X, bias, iters, delta


def _errors(X, bias, Xr, br):
    nz = Xr != 0
    rel_x = float((np.abs(X - Xr)[nz] / np.abs(Xr[nz])).max()) if nz.any() else 0.0
    abs_0 = float(np.abs(X[~nz]).max()) if (~nz).any() else 0.0
    ok = ~np.isnan(br)
    rel_b = float((np.abs(bias[ok] - br[ok]) / np.abs(br[ok])).max()) if ok.any() else 0.0
    return rel_x, abs_0, rel_b


@pytest.mark.parametrize("path", ["default", "inplace"])
@pytest.mark.parametrize("eps,max_iter", ref.SETTINGS)
@pytest.mark.parametrize("n", ref.SIZES)
def test_balance_matches_the_reference(n, eps, max_iter, path, monkeypatch):
    counts, _lay, _short, mask_r, by_rule_r = _case(n)
    Xr, br, iters_r, delta_r, deltas = _reference(n, eps, max_iter)
    # the condition on the inputs, on the reference alone
    assert ref.stop_margin(deltas, eps) >= 1e-6
    if n >= 63:
        assert by_rule_r[1] == 1                                         # the dead bin
    if n == 257:
        assert by_rule_r[0] >= 2                                         # the bins of the two short scaffolds
    if path == "inplace":
        monkeypatch.setenv("HICMI_ICE_INPLACE", "1")
    else:
        monkeypatch.delenv("HICMI_ICE_INPLACE", raising=False)
    mask, by_rule, X, bias, iters, delta = _device(n, eps, max_iter)
    assert np.array_equal(mask, mask_r) and tuple(by_rule) == tuple(by_rule_r)
    assert iters == iters_r
    assert np.array_equal(np.isnan(bias), np.isnan(br)) and np.array_equal(np.isnan(bias), mask_r)
    rel_x, abs_0, rel_b = _errors(X, bias, Xr, br)
    print("n %d eps %g max_iter %d %s: iterations %d, values %.3e relative (%.3e where the reference is 0), biases %.3e, "
          "delta %r against %r" % (n, eps, max_iter, path, iters, rel_x, abs_0, rel_b, delta, delta_r))
    assert rel_x <= BOUND and rel_b <= BOUND
    assert abs_0 <= BOUND * float(np.abs(Xr).max())
    assert abs(delta - delta_r) <= 1e-6 * abs(delta_r)
    # masked rows and columns exactly zero, the result exactly symmetric
    assert not X[mask, :].any() and not X[:, mask].any()
    assert np.array_equal(X, X.T)
    assert np.array_equal(X == 0, np.asarray(Xr) == 0)


@pytest.mark.parametrize("n", [65, 1000])
def test_default_path_is_reproducible_to_the_bit(n, monkeypatch):
    monkeypatch.delenv("HICMI_ICE_INPLACE", raising=False)
    a = _device(n, 1e-6, 100)
    b = _device(n, 1e-6, 100)
    assert a[4] == b[4] and a[5] == b[5]
    assert a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()


def test_mask_rows_zeroes_rows_and_columns():
    from hic_genome_assembler_amd import _lib
    for n in (5, 65, 258):
        rng = np.random.default_rng(n)
        c = rng.random((n, n)) + 1.0
        mask = rng.random(n) < 0.3
        mask[n - 1] = True
        want = c.copy()
        want[mask, :] = 0.0
        want[:, mask] = 0.0
        with _lib.Context(0) as ctx:
            ctx.set_contacts(c)
            ctx.row_sums()
            ctx.ice_mask_rows(mask)
            assert ctx.contacts_host().tobytes() == want.tobytes()
            assert np.allclose(ctx.row_sums()[0], want.sum(axis=1), rtol=1e-13, atol=0)    # the row sums follow the matrix
            with pytest.raises(ValueError):
                ctx.ice_mask_rows(mask[:-1])


def test_adopted_matrix_is_refused_and_untouched():
    import torch
    from hic_genome_assembler_amd import _lib
    counts, _lay, _short, mask, _k = _case(65)
    for ld in (65, 68):
        t = torch.zeros((65, ld), dtype=torch.float64, device="cuda:0")
        t[:, :65] = torch.tensor(np.array(counts), device="cuda:0")
        before = t.clone()
        with _lib.Context(0) as ctx:
            ctx.set_contacts_device(t.data_ptr(), 65, ld, keepalive=t)
            for call in (lambda: ctx.ice_balance(mask, 100, 0.1), lambda: ctx.ice_mask_rows(mask)):
                with pytest.raises(_lib.HicmiError) as exc:
                    call()
                assert "error %d" % ESTATE in str(exc.value)
            torch.cuda.synchronize()
            assert torch.equal(t, before)
            ctx.row_sums()                                               # the context is still usable
            # a compacted copy is the context's own (ld = n_keep): balancing it is allowed and leaves the caller's alone
            ctx.compact(np.arange(64))
            ctx.ice_balance(mask[:64], 5, 0.1)
            torch.cuda.synchronize()
            assert torch.equal(t, before)


def test_bad_arguments():
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        with pytest.raises(_lib.HicmiError):
            ctx.ice_balance(None, 10, 0.1)                               # no matrix
        ctx.set_contacts(np.ones((4, 4)))
        with pytest.raises(_lib.HicmiError):
            ctx.ice_balance(None, 0, 0.1)
        with pytest.raises(_lib.HicmiError):
            ctx.ice_balance(None, 10, -1.0)
        bias, iters, _delta = ctx.ice_balance(None, 10, 0.1)             # no mask: a flat map is balanced at once
        assert iters == 2 and np.array_equal(bias, np.ones(4))
        assert np.array_equal(ctx.contacts_host(), np.ones((4, 4)))


# ---- end to end: -part0 -part1 -part2 ----------------------------------------------------------------------------------
E2E_FILES = ["dendrogramOrder.txt", "binGroups.txt", "assessment.txt", "chromosomeGroups.txt", "chromosomeOrders.txt",
             "plotOrder.txt"]


def _e2e_inputs(work):
    """A 400-bin raw map in the shape of the n400_default fixture (seed 7, 3 chromosomes, scaffolds of 9 bins on
    average), two scaffolds under iceMinScaffoldSize and a dead bin; returns the config path and the HiC-Pro paths."""
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(400, seed=7, n_chrom=3, mean_scaffold_bins=9.0)
    counts, lay = synth.make_raw_counts(lay, seed=7, dead_bins=(123,), short_scaffolds=2, short_size_bp=5000)
    os.makedirs(work)
    paths = synth.write_hicpro(os.path.join(work, "in"), lay, None, raw_counts=counts)
    os.remove(paths["hicProBiasFile"])                                   # -part0 writes these two
    os.remove(paths["hicProMatrixFile"])
    cfg = synth.write_config(os.path.join(work, "config.txt"), paths, os.path.join(work, "out"), os.path.join(work, "plots"),
                             lay.resolution, min_size=5, modularity=0.0, psig=0.05, n_scaffolds=6, scan_scaffolds=5,
                             extra={"hicProRawMatrixFile": paths["hicProRawMatrixFile"], "iceMinScaffoldSize": 10000})
    return cfg, paths


def _texts(work, paths):
    out = {k: open(os.path.join(work, "out", k)).read() for k in E2E_FILES}
    out["biases"] = open(paths["hicProBiasFile"]).read()
    out["matrix"] = open(paths["hicProMatrixFile"]).read()
    return out


def test_part0_hands_its_matrix_to_part1(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import run_hicAssembler as drv
    monkeypatch.setenv("HICMI_LOUVAIN_SEED", "0")
    monkeypatch.delenv("HICMI_ICE_INPLACE", raising=False)
    monkeypatch.delenv("HICMI_ICE_REPARSE", raising=False)
    # one run, the balanced matrix handed over in HBM
    cfg, paths = _e2e_inputs(str(tmp_path / "resident"))
    drv.main(["-part0", "-part1", "-part2", "-config", cfg])
    said = capsys.readouterr().out
    assert "ICE: bins 400, masked" in said and "Edges added to adjacency matrix" in said
    assert said.count("Edges added to adjacency matrix") == 1              # only the raw file was parsed
    resident = _texts(str(tmp_path / "resident"), paths)
    n_bed = open(paths["hicProBedFile"]).read().count("\n")
    assert resident["biases"].count("\n") == n_bed == 400                  # one line per bed line
    assert 3 <= resident["biases"].split("\n").count("nan") < 40
    assert resident["chromosomeOrders.txt"].count("\n") > 20
    # the same with Part 1 parsing the file -part0 wrote
    monkeypatch.setenv("HICMI_ICE_REPARSE", "1")
    cfg, paths = _e2e_inputs(str(tmp_path / "reparse"))
    drv.main(["-part0", "-part1", "-part2", "-config", cfg])
    assert capsys.readouterr().out.count("Edges added to adjacency matrix") == 2
    monkeypatch.delenv("HICMI_ICE_REPARSE")
    assert _texts(str(tmp_path / "reparse"), paths) == resident
    # -part0 alone, then -part1 -part2 in a separate process that reads the written files
    cfg, paths = _e2e_inputs(str(tmp_path / "files"))
    drv.main(["-part0", "-config", cfg])
    res = subprocess.run([sys.executable, os.path.join(ROOT, "run_hicAssembler.py"), "-part1", "-part2", "-config", cfg],
                         env=dict(os.environ), capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    assert _texts(str(tmp_path / "files"), paths) == resident
