"""The Part 1 HMM sweep (sweepHMM.py) on the CPU: grid parsing, names, refusals, the generator form of
identifyChromosomeGroupsHMM against recorded digests and the literal restatement, and the lock-step planner's sharing of
fits."""
import contextlib
import hashlib
import io
import json
import os

import numpy as np
import pytest

import hmm_reference as ref
from test_sweep_cpu import _config

PATHS = {k: "x" for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}


def test_grid_parsing_and_names(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run, sweepHMM as sw
    v = run.readConfigFileToVariables(_config(tmp_path, PATHS, hyperGeom="False", hmm="True", lookAhead="False"))
    assert v["lookAhead"] is False
    args = sw._parse_args(["-config", "c", "-minSize", "5,10,5", "-modularity", ".05,.1", "-convergenceRounds", "5,8",
                           "-lookAhead", ".2,False,.5"])
    minSizes, mods, crs, las, lrs = sw.grid_from_args(args, v)
    assert (minSizes, mods, crs, lrs) == ([5, 10], [.05, .1], [5, 8], [20])
    assert las == [.2, False, .5]
    grid = sw.settings(minSizes, crs, las, mods, lrs)
    assert len(grid) == 2 * 2 * 3 * 2 and grid[0] == (5, 5, .2, .05, 20) and grid[1] == (5, 5, .2, .1, 20)
    assert sw.setting_name(5, 8, .2, .05) == "minSize5_convergenceRounds8_lookAhead0.2_modularity0.05"
    assert sw.setting_name(10, 5, False, 0.0, 20) == "minSize10_convergenceRounds5_lookAheadFalse_modularity0_louvainRounds20"
    assert len({sw.setting_name(*g) for g in grid}) == len(grid)


def test_refusals(tmp_path, capsys, monkeypatch):
    from hic_genome_assembler_amd import run_hicAssembler as run, sweepHMM as sw
    monkeypatch.setenv("HICMI_HMM", "1")
    v = run.readConfigFileToVariables(_config(tmp_path, PATHS, hyperGeom="True", hmm="False"))
    assert "hmm = True and hyperGeom = False" in sw.check_config(v)
    v = run.readConfigFileToVariables(_config(tmp_path, PATHS, hyperGeom="False", hmm="True"))
    assert sw.check_config(v) is None
    with pytest.raises(SystemExit):
        sw.main(["-config", _config(tmp_path, PATHS, hyperGeom="True", hmm="False")])
    assert "hyperGeom = False" in capsys.readouterr().out
    monkeypatch.delenv("HICMI_HMM")
    assert "HICMI_HMM=1" in sw.check_config(v)
    with pytest.raises(SystemExit):
        sw.main(["-config", _config(tmp_path, PATHS, hyperGeom="False", hmm="True")])
    assert "HICMI_HMM=1" in capsys.readouterr().out
    with pytest.raises(NotImplementedError, match="HICMI_HMM=1"):
        sw.runSweep(*(["x"] * 8), [5], [.05], [5], [.2], [20], str(tmp_path))
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        sw.main([])                                          # no -config


def _scripted(seed):
    """hmm_states of a fake matrix: a step from state 0 to 1 at a position drawn from (c, width, call number), or no
    step at all (no boundary)."""
    def states(c, width, idx, n):
        rng = np.random.default_rng([seed, c, width, idx])
        T = n - c
        k = int(rng.integers(1, T)) if rng.uniform() < .85 else T
        if rng.uniform() < .3:
            k = int(rng.integers(1, 8))                      # a step close to c: narrow next rounds
        return np.array([0] * k + [1] * (T - k), np.int32)
    return states


class _FakeMatrix:
    def __init__(self, n, fn):
        self.n, self.fn, self.calls = n, fn, []

    def __len__(self):
        return self.n

    def hmm_states(self, c, p):
        self.calls.append((c, p - c))
        return self.fn(c, p - c, len(self.calls) - 1, self.n)


def _strip(lines):
    from hic_genome_assembler_amd import sweepHMM as sw
    return [ln for ln in "\n".join(lines).split("\n") if not sw._is_hmm_runtime_line(ln)]


# n x seed x minSize x modularity x convergenceRounds x lookAhead; tests/golden/hmm_groups_digests.json holds one digest
# per case in this order, recorded from the function before it was driven by the generator
HMM_GRID = [(n, seed, ms, mod, cr, la) for n in (40, 90, 300) for seed in range(6) for ms in (3, 5, 12)
            for mod in (0.0, .05, .3, 1) for cr in (1, 2, 4) for la in (False, .2, .5, 1.0)]
HMM_DIGESTS = os.path.join(os.path.dirname(__file__), "golden", "hmm_groups_digests.json")


def _digest(cuts, calls, lines):
    """12 hex digits of the cut list, the (c, width) requests and the printed lines (run-time lines stripped)."""
    blob = json.dumps([cuts, [list(k) for k in calls], lines])
    return hashlib.sha256(blob.encode()).hexdigest()[:12]


def _run_identify(n, seed, ms, mod, cr, la):
    """identifyChromosomeGroupsHMM on a scripted matrix: (cuts, requests, printed lines without run-time lines)."""
    from hic_genome_assembler_amd import scaffoldToChromosomes as s2c
    fm = _FakeMatrix(n, _scripted(seed))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cuts = s2c.identifyChromosomeGroupsHMM(fm, None, minSize=ms, modularity=mod, convergenceRounds=cr, lookAhead=la)
    return cuts, fm.calls, _strip(buf.getvalue().splitlines())


def test_generator_equals_identifyChromosomeGroupsHMM():
    """identifyChromosomeGroupsHMM (the generator driven with print) matches the recorded digests of the function it
    replaced, the literal restatement in hmm_reference.py on cuts and requests, and the generator driven by hand on
    cuts, requests, fit indices and lines."""
    from hic_genome_assembler_amd import scaffoldToChromosomes as s2c
    with open(HMM_DIGESTS) as fh:
        digests = json.load(fh)
    assert len(digests) == len(HMM_GRID)
    seen = set()
    for (n, seed, ms, mod, cr, la), digest in zip(HMM_GRID, digests):
        case = (n, seed, ms, mod, cr, la)
        want, calls, printed = _run_identify(*case)
        assert _digest(want, calls, printed) == digest, case
        ref_backend = _FakeMatrix(n, _scripted(seed))
        assert ref.identifyChromosomeGroupsHMM(ref_backend, ms, mod, cr, la) == want, case
        assert ref_backend.calls == calls, case
        lines, reqs = [], []
        fn = _scripted(seed)

        def serve(c, width, fit_index):
            reqs.append((c, width))
            assert fit_index == len(reqs) - 1
            return fn(c, width, fit_index, n)
        got = s2c.drive(s2c.hmm_groups_steps(n, minSize=ms, modularity=mod, convergenceRounds=cr, lookAhead=la,
                                             emit=lines.append), serve)
        assert got == want, case
        assert reqs == calls
        assert _strip(lines) == printed
        text = "\n".join(printed)
        seen.update(k for k, s in (("NA", "'NA']"), ("noconv", "failed to converge"),
                                   ("pop", "Last cut index found to be length"),
                                   ("recurse", "Recursing on identifyChromosomeGroupsHMM"),
                                   ("terminated", "Algorithm terminated"))
                    if s in text)
        if mod == 1:
            assert got == [] and not reqs
            seen.add("mod1")
        if mod == 0.0:
            seen.add("mod0")
    assert seen >= {"NA", "noconv", "pop", "recurse", "terminated", "mod0", "mod1"}, seen


def test_planner_shares_fits():
    from hic_genome_assembler_amd import scaffoldToChromosomes as s2c, sweepHMM as sw
    keys, widest = sw.plan_round({0: (0, 60, 0), 1: (0, 60, 0), 2: (0, 30, 0), 3: (40, 20, 1), 4: (0, 60, 0)})
    assert keys == [(0, 60, 0), (0, 30, 0), (40, 20, 1)]
    assert widest == {0: 60, 40: 20}
    n = 300
    fn = _scripted(3)

    class Fitter:
        def __init__(self):
            self.made = []

        def fit(self, keys, widest):
            for k in keys:
                assert widest[k[0]] >= k[1]
            self.made += keys
            return {k: fn(k[0], k[1], k[2], n) for k in keys}

    grid = sw.settings([5, 8], [2, 4], [.2, .5], [.05, .1], [20])
    f = Fitter()
    found = sw.run_lock_step(n, grid, f)
    assert len(f.made) == len(set(f.made)) == sum(x[3] for x in found)
    for (ms, cr, la, mod, lr), (cuts, lines, n_req, n_run) in zip(grid, found):
        fm = _FakeMatrix(n, fn)
        with contextlib.redirect_stdout(io.StringIO()):
            want = s2c.identifyChromosomeGroupsHMM(fm, None, minSize=ms, modularity=mod, convergenceRounds=cr, lookAhead=la)
        assert cuts == want and n_req == len(fm.calls)
    # settings that differ only in modularity ask for the same first fits: every modularity .1 setting shares its
    # first fit with the .05 one before it
    total_req = sum(x[2] for x in found)
    assert sum(x[3] for x in found) < total_req
    for i in range(0, len(grid), 2):
        assert found[i + 1][2] >= 1 and found[i + 1][3] < found[i + 1][2]


def test_slot_batches_respect_the_budget(monkeypatch):
    from hic_genome_assembler_amd import sweepHMM as sw
    n = 1000
    widest = {0: 200, 100: 500, 400: 600, 900: 100}
    batches = sw._slot_batches(n, widest, 3_000_000)
    assert sorted(c for b in batches for c in b) == sorted(widest)
    for b in batches:
        assert len(b) == 1 or sum((n - c) * widest[c] * 8 for c in b) <= 3_000_000
    assert len(sw._slot_batches(n, widest, 1 << 40)) == 1
    many = {c: 10 for c in range(0, 900, 30)}
    assert all(len(b) <= 16 for b in sw._slot_batches(n, many, 1 << 40))


def test_module_docs_and_summary_columns():
    from hic_genome_assembler_amd import sweepHMM as sw
    assert {"fits_requested", "fits_run", "cut_indices", "convergenceRounds", "lookAhead"} <= set(sw.SUMMARY_COLUMNS)
    assert os.path.basename(sw.__file__) == "sweepHMM.py"
