"""The multi-set scan loops (hicmi_first_pass_cuts_multi / hicmi_filter_cuts_multi) against the single-set calls, set by
set, and the Part 1 sweep (sweepPart1.runSweep) against separate -part1 runs on a real MI355X."""
import os

import numpy as np
import pytest

import golden_cases as gc

pytestmark = pytest.mark.gpu

FILES = ("binGroups.txt", "assessment.txt", "chromosomeGroups.txt")
SCAN_PREFIXES = ("- M value", "- Breakpoints found", "- WARNING - Maximum number of rounds", "- Original cut indices",
                 "- Filtered cut indices")


@pytest.fixture(scope="module")
def hic():
    from hic_genome_assembler_amd import _lib
    _lib.load()
    return _lib


def _ranked(hic, c):
    ctx = hic.Context(0)
    ctx.set_contacts(np.ascontiguousarray(c, dtype=np.float64))
    leaves, _z = ctx.upgma()
    ctx.rank_matrix(leaves)
    return ctx


def _golden_contacts(name):
    _spec, _meta, _gold, _lay, c = gc.load_case(name)
    c = np.asarray(c, np.float64)
    keep = c.sum(axis=1) != 0                                # (removeRows: n300_edges has empty rows)
    return np.ascontiguousarray(c[keep][:, keep])


def _check_sets(ctx, first_sets, psigs):
    """Every first-pass set and every (its cuts, psig) filter set through the multi entries and one by one."""
    multi = ctx.first_pass_cuts_multi(first_sets, .05)
    assert len(multi) == len(first_sets)
    lists = []
    for (ms, stop), got in zip(first_sets, multi):
        assert got == ctx.first_pass_cuts(ms, stop, .05), (ms, stop)
        if got[0] and got[0] not in lists:
            lists.append(got[0])
    fsets = [(lst, ps) for lst in lists for ps in psigs]
    if fsets:
        multi = ctx.filter_cuts_multi([s[0] for s in fsets], [s[1] for s in fsets])
        for (lst, ps), got in zip(fsets, multi):
            assert got == ctx.filter_cuts(lst, ps), (lst, ps)
    return lists


@pytest.mark.parametrize("name", ["n300_edges", "n400_default", "n500_sparse", "n2000"])
def test_multi_equals_single_on_golden_maps(hic, name):
    c = _golden_contacts(name)
    n = len(c)
    sets = [(ms, int(n - n * mf)) for ms in (1, 3, 5, 8) for mf in (0.0, .05, .2)]
    with _ranked(hic, c) as ctx:
        lists = _check_sets(ctx, sets, (.05, .01, .001))
        assert lists


@pytest.mark.parametrize("n,seed", [(3000, 3), (8000, 4)])
def test_multi_equals_single_on_synthetic_maps(hic, n, seed):
    """minSize {1,3,5,8,12,15} x min_frac {0,.05,.2,.5}: sets that end after very different scan counts share one batch;
    then a filter batch that mixes short lists with one of more than 2,048 candidates (the global-memory path)."""
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(n, seed=seed)
    c = synth.dense_contacts(lay, seed=seed)
    sets = [(ms, int(n - n * mf)) for ms in (1, 3, 5, 8, 12, 15) for mf in (0.0, .05, .2, .5)]
    with _ranked(hic, c) as ctx:
        lists = _check_sets(ctx, sets, (.05, .01, .001))
        counts = [len(ctx.first_pass_cuts(ms, st, .05)[0]) for ms, st in sets]
        assert max(counts) > min(counts)                      # (the sets end after different numbers of scans)
        dense = list(range(40, n - 40, 40))
        mixed = [lists[0], dense, [], lists[-1]]
        if n == 8000:
            very_dense = list(range(6, n - 6, 3))
            assert len(very_dense) > 2048
            mixed.append(very_dense)
        psigs = [.05, .01, .05, .001] + ([.05] if n == 8000 else [])
        got = ctx.filter_cuts_multi(mixed, psigs)
        for lst, ps, g in zip(mixed, psigs, got):
            assert g == (ctx.filter_cuts(lst, ps) if lst else ([], 0)), (len(lst), ps)


def test_multi_set_counts_and_cap(hic):
    c = _golden_contacts("n400_default")
    n = len(c)
    with _ranked(hic, c) as ctx:
        one = ctx.first_pass_cuts(5, int(n - n * .05), .05)
        assert ctx.first_pass_cuts_multi([(5, int(n - n * .05))], .05) == [one]       # n_sets = 1
        dup = ctx.first_pass_cuts_multi([(5, n), (3, n), (5, n), (5, n)], .05)         # duplicate sets
        assert dup[0] == dup[2] == dup[3] == ctx.first_pass_cuts(5, n, .05)
        assert dup[1] == ctx.first_pass_cuts(3, n, .05)
        cap = hic.Context.SCAN_MAX_SETS
        sets = [(1 + k % 9, n - 7 * (k // 9)) for k in range(cap)]                  # exactly the cap, in one call
        assert len(set(sets)) == cap
        got = ctx.first_pass_cuts_multi(sets, .05)
        for s, g in zip(sets, got):
            assert g == ctx.first_pass_cuts(s[0], s[1], .05), s
        lists = [one[0]] * cap
        psigs = [(.05, .01, .001)[k % 3] for k in range(cap)]
        got = ctx.filter_cuts_multi(lists, psigs)
        for ps, g in zip(psigs[:3], got[:3]):
            assert g == ctx.filter_cuts(one[0], ps)
        assert all(g == got[k % 3] for k, g in enumerate(got))
        # more sets than the cap: the entry point refuses, the Context method splits into chunks
        import ctypes
        ms = np.full(cap + 1, 5, np.int64)
        st = np.full(cap + 1, n, np.int64)
        buf = np.empty((cap + 1, n), np.int32)
        cnt = np.empty(cap + 1, np.int64)
        mlog = np.empty((cap + 1, n, 2), np.int32)
        rc = ctx._lib.hicmi_first_pass_cuts_multi(ctx._h, cap + 1, ms.ctypes.data, st.ctypes.data, ctypes.c_double(.05),
                                                  buf.ctypes.data, n, cnt.ctypes.data, mlog.ctypes.data, n, cnt.ctypes.data)
        assert rc == -1
        assert ctx.first_pass_cuts_multi([(5, n)] * (cap + 1), .05) == [ctx.first_pass_cuts(5, n, .05)] * (cap + 1)


def test_shared_counts_do_not_change_results(hic, monkeypatch):
    """HICMI_SCAN_SHARE=0 (every set counts its own rows) gives the same outputs as the default."""
    c = _golden_contacts("n2000")
    n = len(c)
    sets = [(ms, int(n - n * mf)) for ms in (3, 5, 8) for mf in (0.0, .05)]
    with _ranked(hic, c) as ctx:
        a = ctx.first_pass_cuts_multi(sets, .05)
        fl = ctx.filter_cuts_multi([a[0][0]] * 3, [.05, .01, .001])
        monkeypatch.setenv("HICMI_SCAN_SHARE", "0")
        assert ctx.first_pass_cuts_multi(sets, .05) == a
        assert ctx.filter_cuts_multi([a[0][0]] * 3, [.05, .01, .001]) == fl


def _scan_lines(lines):
    return [ln for ln in lines if ln.startswith(SCAN_PREFIXES)]


@pytest.mark.parametrize("device_louvain", [False, True])
def test_sweep_equals_separate_runs(hic, tmp_path, capsys, monkeypatch, device_louvain):
    import hic_oracle as orc
    from hic_genome_assembler_amd import scaffoldToChromosomes as p1, sweepPart1 as sw
    if device_louvain:
        monkeypatch.setenv("HICMI_LOUVAIN_DEVICE", "1")
    else:
        monkeypatch.delenv("HICMI_LOUVAIN_DEVICE", raising=False)
    name = "n400_default"
    paths = gc.write_case_files(name, str(tmp_path))
    out = str(tmp_path / "sweep")
    f = lambda d, k: os.path.join(d, k)  # noqa: E731
    grid = ([3, 5, 8], [.05, .01], [0.0, .05])
    sw.runSweep(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], paths["hicProScaffSizeFile"],
                str(tmp_path / "dendrogramOrder.txt"), "binGroups.txt", "assessment.txt", "chromosomeGroups.txt",
                *grid, [20], out)
    rows = sw.read_summary(os.path.join(out, "sweep_summary.tsv"))
    for (ms, ps, mod, lr), row in zip(sw.combinations(*grid, [20]), rows):
        d = os.path.join(out, sw.combo_name(ms, ps, mod))
        ref = tmp_path / ("run_%d_%g_%g" % (ms, ps, mod))
        ref.mkdir()
        capsys.readouterr()
        p1.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                       paths["hicProScaffSizeFile"], f(ref, "dendrogramOrder.txt"), f(ref, "a.png"), f(ref, "b.png"),
                       f(ref, "binGroups.txt"), f(ref, "assessment.txt"), f(ref, "chromosomeGroups.txt"),
                       True, False, ms, mod, lr, ps, 5, .2, 100000)
        printed = capsys.readouterr().out.splitlines()
        for fn in FILES:
            with open(f(d, fn)) as a, open(f(ref, fn)) as b:
                assert a.read() == b.read(), (ms, ps, mod, fn)
        with open(f(d, "part1.log")) as fh:
            log = fh.read().splitlines()
        assert _scan_lines(log) == _scan_lines(printed), (ms, ps, mod)
        final = [ln for ln in printed if ln.startswith("CutIndices = ")][-1]
        assert row["cut_indices"] == [int(v) for v in final.split("=", 1)[1].strip(" []").split(",") if v.strip()]
        if mod == 0.0:
            o = tmp_path / ("oracle_%d_%g" % (ms, ps))
            o.mkdir()
            orc.run_part1(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                          paths["hicProScaffSizeFile"], f(o, "d.txt"), f(o, "binGroups.txt"), f(o, "assessment.txt"),
                          f(o, "chromosomeGroups.txt"), min_size=ms, modularity=0.0, psig=ps)
            for fn in FILES:
                with open(f(d, fn)) as a, open(f(o, fn)) as b:
                    assert a.read() == b.read(), (ms, ps, fn)
        else:
            assert int(row["louvain_groups"]) >= 1


def test_multi_equals_single_at_bench_scale(hic):
    """bench.py's 16k synthetic map (seed=1, sinkhorn_iters=12), a 16-set first-pass grid and its filter sets."""
    import torch
    from hic_genome_assembler_amd import synth
    n = 16000
    lay = synth.make_layout(n, seed=1)
    c = synth.dense_contacts_torch(lay, torch.device("cuda:0"), seed=1, sinkhorn_iters=12).cpu().numpy()
    sets = [(ms, int(n - n * mf)) for ms in (5, 8, 10, 15) for mf in (0.0, .05, .2, .5)]
    with _ranked(hic, c) as ctx:
        del c
        lists = _check_sets(ctx, sets, (.05, .01, .001))
        assert len(lists) >= 4
