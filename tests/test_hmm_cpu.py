"""The HMM boundary finder (hmm = True, S2C:730-942) without a GPU: the host control flow of scaffoldToChromosomes
against the literal restatement in hmm_reference.py on scripted state vectors, the restatement's k-means against
sklearn (where it imports) and its EM's monotone log-likelihood, and the HICMI_HMM opt-in."""
import contextlib
import io
import os

import numpy as np
import pytest

import hmm_reference as ref
from hic_genome_assembler_amd import run_hicAssembler as run
from hic_genome_assembler_amd import scaffoldToChromosomes as p1


class Scripted:
    """A fit-and-decode backend whose states come from ``fn(c, p, call)``."""

    def __init__(self, n, fn):
        self.n, self.fn, self.calls = n, fn, []

    def __len__(self):
        return self.n

    def hmm_states(self, c, p):
        self.calls.append((c, p))
        return np.asarray(self.fn(c, p, len(self.calls) - 1), dtype=np.int32)


def planted(bounds):
    """States 0 up to the first planted boundary after c, 1 from there on."""
    def fn(c, p, _call):
        n = bounds[-1]
        b = next((x for x in bounds if x > c), n)
        s = np.ones(n - c, np.int32)
        s[:b - c] = 0
        return s
    return fn


def both(n, fn, **kw):
    """(product cuts, restatement cuts, product calls, restatement calls) for the same scripted backend."""
    a, b = Scripted(n, fn), Scripted(n, fn)
    with contextlib.redirect_stdout(io.StringIO()):
        got = p1.identifyChromosomeGroupsHMM(a, None, **kw)
    want = ref.identifyChromosomeGroupsHMM(b, **{k: v for k, v in kw.items() if k != "louvainRounds"})
    return got, want, a.calls, b.calls


def test_identify_boundary_windows_and_ties():
    rng = np.random.default_rng(5)
    cases = [([0] * 5 + [1] * 5, 2), ([1, 1, 0, 0] + [0] * 6 + [1] * 3, 2), ([0, 1] * 6 + [1] * 4, 4),
             ([1] * 3 + [0] * 10, 3), ([0] * 10 + [1] * 10, 10), ([0] * 3, 5), ([1] * 12, 4), ([0] * 10 + [1] * 4, 4)]
    for _ in range(200):
        k = int(rng.integers(1, 8))
        cases.append((list(rng.integers(0, 2, size=int(rng.integers(0, 40)))), k))
        m = int(rng.integers(k, 30))
        cases.append(([0] * m + [1] * int(rng.integers(0, 30)), k))
    for states, k in cases:
        for cuts in ([0], [0, 17]):
            assert p1.identifyBoundry(np.array(states, np.int32), cuts, k) == ref.identifyBoundry(states, cuts, k), (states, k)
    # a tie in the first window starts in state 0; the last window is not looked at
    assert p1.identifyBoundry([0, 1, 1, 1, 1, 1], [0], 2) == 1
    assert p1.identifyBoundry([0, 0, 1, 1], [0], 2) == 0


def test_planted_boundaries_and_recursion_on_a_final_cut():
    n = 1000
    got, want, calls, _ = both(n, planted([300, 700, 960, n]), minSize=5, modularity=.05, convergenceRounds=5,
                               lookAhead=.2)
    assert got == want == [300, 700, 960]                  # 960 > n - .05 n ends the loop
    assert calls[0] == (0, 200)                             # lookAhead resolved against n - c: int(1000 * .2)
    assert calls[1] == (0, 300)                             # the second round of a boundary reads up to the last cut
    # modularity 0: the loop runs to the end of the matrix and stops on "NA"
    got, want, _, _ = both(n, planted([300, 700, 990, n]), minSize=5, modularity=0.0, convergenceRounds=5, lookAhead=.2)
    assert got == want and got[:3] == [300, 700, 990]
    # a boundary before the modularity tail with no switch after it: the fit of the tail gives cut 0, which ends the
    # loop - and stays in the list, as in the reference
    got, want, _, _ = both(n, planted([300, 700, 900, n]), minSize=5, modularity=.05, convergenceRounds=5, lookAhead=.2)
    assert got == want == [300, 700, 900, 0]


def test_non_convergence_and_the_cut_equal_to_n():
    n = 400

    def moving(c, p, call):                              # the boundary moves with every fit: rounds run out
        s = np.zeros(n - c, np.int32)
        s[min(n - c - 6, 20 + 7 * call):] = 1
        return s
    got, want, _, _ = both(n, moving, minSize=5, modularity=.05, convergenceRounds=3, lookAhead=.5)
    assert got == want and len(got) >= 1

    def never(c, p, call):                               # no switch at all: 0, then the width < minSize branch -> n
        return np.zeros(n - c, np.int32)
    out = io.StringIO()
    a = Scripted(n, never)
    with contextlib.redirect_stdout(out):
        got = p1.identifyChromosomeGroupsHMM(a, None, minSize=5, modularity=.05, convergenceRounds=2, lookAhead=False)
    want = ref.identifyChromosomeGroupsHMM(Scripted(n, never), 5, .05, 2, False)
    assert got == want == []                             # [0, n] -> [n] -> []: the reference raises IndexError here
    assert "WARNING - no chromosome boundary left" in out.getvalue()

    def once_then_never(c, p, call):                     # one boundary, then a final cut at n: the recursion
        s = np.zeros(n - c, np.int32)
        if c == 0:
            s[100:] = 1
        return s
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        got, want, calls, rcalls = both(n, once_then_never, minSize=5, modularity=.05, convergenceRounds=4, lookAhead=False)
    assert got == want and got[0] == 100 and calls == rcalls
    assert (100, 250) in calls                           # the recursion's lookAhead .5: int(300 * .5) + 100


def test_na_and_narrow_windows():
    # (n - c) / 2 < minSize at once: "NA", popped, then the leading 0: nothing left
    got, want, calls, _ = both(16, planted([8, 16]), minSize=10, modularity=.05, convergenceRounds=5, lookAhead=.2)
    assert got == want == [] and calls == []
    # len(X[0]) < minSize: cutInd = lookAhead (absolute), no fit for that round
    got, want, calls, rcalls = both(200, planted([100, 200]), minSize=50, modularity=.05, convergenceRounds=5,
                                    lookAhead=.2)
    assert got == want and calls == rcalls
    assert all(p - c >= 50 for c, p in calls)


def test_kmeans_restatement_matches_sklearn():
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(3)
    for T, D in ((2, 1), (63, 5), (500, 40), (300, 1)):
        X = rng.normal(size=(T, D))
        X[: T // 2] += 3.0
        init = X[[0, T - 1]]
        km = cluster.KMeans(n_clusters=2, init=init, n_init=1, algorithm="lloyd", tol=1e-4).fit(X)
        tol = 1e-4 * float(np.mean(X.var(axis=0)))
        centers, labels, inertia, it = ref.kmeans_lloyd(X, init, 300, tol)
        assert np.array_equal(labels, km.labels_)
        assert np.allclose(centers, km.cluster_centers_, rtol=1e-10, atol=1e-12)
        assert inertia == pytest.approx(km.inertia_, rel=1e-10)


def test_em_never_decreases_logprob():
    rng = np.random.default_rng(11)
    for T, D in ((2, 1), (40, 3), (300, 12), (1000, 30)):
        X = rng.normal(size=(T, D))
        X[T // 3:] += rng.normal(size=D)
        means, covars, _ = ref.init_params(X, 0, 0)
        _m, _c, A, hist = ref.fit(X, means, covars, ref.TRANSMAT, tol=-np.inf, n_iter=30)
        assert np.all(np.diff(hist) >= -1e-9 * np.abs(hist[1:])), hist
        assert np.allclose(A.sum(axis=1), 1.0)
        states = ref.viterbi(X, _m, _c, A)
        assert states.shape == (T,) and set(np.unique(states)) <= {0, 1}


def _hmm_config(tmp_path):
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(200, seed=3)
    c = synth.dense_contacts(lay, seed=3)
    d = tmp_path / "in"
    d.mkdir()
    paths = synth.write_hicpro(str(d), lay, c)
    cfg = tmp_path / "c.txt"
    synth.write_config(str(cfg), paths, str(tmp_path / "o"), str(tmp_path / "p"), lay.resolution)
    text = cfg.read_text().replace("hmm = False", "hmm = True").replace("hyperGeom = True", "hyperGeom = False")
    cfg.write_text(text)
    return cfg


def test_opt_in_switch(tmp_path, monkeypatch):
    cfg = _hmm_config(tmp_path)
    v = run.readConfigFileToVariables(str(cfg))
    assert v["hmm"] is True and v["hyperGeom"] is False
    monkeypatch.delenv("HICMI_HMM", raising=False)
    assert run.ensureAllVariablesAreSet(v) is True
    monkeypatch.setenv("HICMI_HMM", "1")
    assert run.ensureAllVariablesAreSet(v) is False
    both_false = dict(v, hmm=False)
    assert run.ensureAllVariablesAreSet(both_false) is True             # still refused (the reference: NameError)
    both_true = dict(v, hyperGeom=True)
    assert run.ensureAllVariablesAreSet(both_true) is True
    # past the refusal, runPipeline goes on to read the inputs (here: files that do not exist)
    with pytest.raises((FileNotFoundError, OSError)):
        p1.runPipeline(*([str(tmp_path / "missing")] * 10), False, True, 5, 0.05, 20, .05, 5, .2, 100000)
    with pytest.raises(NotImplementedError):
        p1.runPipeline(*([str(tmp_path / "missing")] * 10), False, False, 5, 0.05, 20, .05, 5, .2, 100000)


def test_opt_in_through_main(tmp_path, monkeypatch):
    """run.main with HICMI_HMM=1 passes the config check and enters Part 1.  Without a GPU the first device call is
    where it stops; with one, the 200-bin run completes and writes its files."""
    cfg = _hmm_config(tmp_path)
    monkeypatch.setenv("HICMI_HMM", "1")
    out = io.StringIO()
    err = None
    with contextlib.redirect_stdout(out):
        try:
            run.main(["-part1", "-config", str(cfg)])
        except Exception as exc:                           # no device here
            err = exc
    assert not isinstance(err, NotImplementedError)
    assert "Working on Part1" in out.getvalue()
    if err is None:
        assert "Working on iterative 2 state HMMs" in out.getvalue()
        for fn in ("dendrogramOrder.txt", "binGroups.txt", "assessment.txt", "chromosomeGroups.txt"):
            assert os.path.getsize(str(tmp_path / "o" / fn)) > 0
