"""The HMM boundary finder (hmm = True, S2C:730-942) on the GPU: the observation build against the log-transformed
similarity, k-means / Baum-Welch / Viterbi against the NumPy restatement (hmm_reference.py), and the whole Part 1 with
HICMI_HMM=1 on synthetic maps."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

import hmm_reference as ref

pytestmark = pytest.mark.gpu


def _map(n, seed=1):
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(n, seed=seed)
    return lay, synth.dense_contacts(lay, seed=seed)


@pytest.fixture(scope="module")
def map2000():
    from hic_genome_assembler_amd import _lib
    lay, C = _map(2000)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(C)
        ctx.row_sums()
        leaves, _z = ctx.upgma(want_linkage=False)
    leaves = np.asarray(leaves)
    return lay, C, leaves, ref.log_similarity(C, leaves)


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


@pytest.mark.parametrize("n", [600, 2000])
def test_observations_equal_the_log_similarity(n):
    from hic_genome_assembler_amd import _lib
    _lay, C = _map(n, seed=2)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(C)
        ctx.row_sums()
        leaves, _z = ctx.upgma(want_linkage=False)
        A = ref.log_similarity(C, np.asarray(leaves))
        for c, p in ((0, n), (0, 40), (n // 3, n // 3 + 63), (n // 5, n - 7), (17, 17 + 1100 if n > 1200 else n), (n - 30, n)):
            ctx.hmm_load_obs(leaves, c, p)
            X = ctx.hmm_get_obs()
            want = A[c:, c:p]
            assert X.shape == want.shape
            assert int(_ulps(X, want).max()) <= 2, (c, p)
            if p - c > 10:                                   # a narrower view of the same X
                ctx.hmm_set_width(p - c - 10)
                assert np.array_equal(ctx.hmm_get_obs(3, 5), X[3:8, :p - c - 10])


def _planted(T, D, rng):
    X = rng.normal(scale=.3, size=(T, D))
    X[: T // 2] += 1.0
    return X


def _cases(map2000):
    rng = np.random.default_rng(7)
    A = map2000[3]
    return [("planted", _planted(2, 1, rng)), ("planted", _planted(63, 7, rng)), ("random", rng.normal(size=(300, 64))),
            ("planted", _planted(1000, 257, rng)), ("planted", _planted(16385, 3, rng)),
            ("planted", _planted(700, 4097, rng)), ("synth", A[0:, 0:400]), ("synth", A[900:, 900:1160]),
            ("synth", A[1800:, 1800:1840])]


def test_kmeans_fit_decode_match_the_restatement(map2000):
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as p1
    with _lib.Context(0) as ctx:
        for name, X in _cases(map2000):
            T, D = X.shape
            ctx.hmm_set_obs(X)
            # k-means from given centers
            rng = np.random.default_rng([1, T, D])
            rows = ref.kmeans_plusplus_rows(X, rng)
            tol = 1e-4 * float(np.mean(X.var(axis=0)))
            c_ref, l_ref, in_ref, it_ref = ref.kmeans_lloyd(X, X[rows], 300, tol)
            c_gpu, l_gpu, in_gpu, it_gpu = ctx.hmm_kmeans(X[rows], 300, tol)
            assert np.array_equal(l_gpu, l_ref) and it_gpu == it_ref, name
            assert np.allclose(c_gpu, c_ref, rtol=1e-12, atol=1e-14), name
            assert in_gpu == pytest.approx(in_ref, rel=1e-12, abs=1e-14)
            if T < 4:
                continue
            # the seeded initialisation of the device path
            means_g, covars_g = p1.hmm_init_params(ctx, T, 0, 3)
            means_r, covars_r, _ = ref.init_params(X, 0, 3)
            assert np.allclose(means_g, means_r, rtol=1e-12, atol=1e-14), name
            assert np.allclose(covars_g, covars_r, rtol=1e-12, atol=1e-14), name
            # Baum-Welch from the same initial parameters, then Viterbi
            mr, vr, ar, hr = ref.fit(X, means_r, covars_r, ref.TRANSMAT)
            mg, vg, ag, hg = ctx.hmm_fit(ref.STARTPROB, means_r, covars_r, ref.TRANSMAT, ref.N_ITER, ref.TOL)
            assert len(hg) == len(hr), name
            assert np.allclose(hg, hr, rtol=1e-9, atol=0), name
            for g, r in ((mg, mr), (vg, vr), (ag, ar)):
                assert np.allclose(g, r, rtol=1e-9, atol=1e-9), name
            s_ref = ref.viterbi(X, mr, vr, ar)
            assert np.array_equal(ctx.hmm_decode(ref.STARTPROB, mr, vr, ar), s_ref), name
            assert np.array_equal(ctx.hmm_decode(ref.STARTPROB, mg, vg, ag), s_ref), name


def _device_matrix(ctx, C, leaves):
    from hic_genome_assembler_amd import scaffoldToChromosomes as p1
    ctx.set_contacts(C)
    ctx.row_sums()
    m = p1.DeviceMatrix(ctx)
    m.order = list(leaves)
    m.kind = "similarity"
    return m


@pytest.mark.parametrize("modularity", [0.0, .05])
def test_hmm_cuts_match_the_restatement_at_2000_bins(map2000, modularity):
    """The boundaries of identifyChromosomeGroupsHMM on the device equal those of the restatement with the same seed.
    Against the hyperGeom finder on the same map: every planted boundary either finds, the HMM finds too.  Away from
    them the two finders disagree (the hyperGeom scans also cut inside a small chromosome at
    modularity 0, the HMM splits the last chromosome at .05), so those cuts are not compared."""
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as p1
    lay, C, leaves, A = map2000
    be = ref.NumpyBackend(A, seed=0)
    want = ref.identifyChromosomeGroupsHMM(be, 5, modularity, 5, .2)
    with _lib.Context(0) as ctx, contextlib.redirect_stdout(io.StringIO()):
        m = _device_matrix(ctx, C, leaves)
        got = p1.identifyChromosomeGroupsHMM(m, None, minSize=5, modularity=modularity, convergenceRounds=5, lookAhead=.2)
        assert m.hmm.stats["fits"] == len(be.log)
        assert m.hmm.stats["builds"] < m.hmm.stats["fits"]          # later rounds of a boundary reuse X
        ctx.rank_matrix(leaves)
        rank = p1.RankMatrix(ctx)
        hyper = p1.filter_noisy_breakpoints(rank, p1.pre_process_all_matrix_breakpoints(rank, 5, modularity, .05), .05)
    assert got == want
    chrom = lay.chrom_of_bin[leaves]
    planted = list(np.flatnonzero(np.diff(chrom)) + 1)
    assert all(b in got for b in planted), (planted, got)
    for b in planted:
        if min(abs(b - h) for h in hyper) <= 5:
            assert min(abs(b - g) for g in got) <= 5, (b, got, hyper)
    print("planted %s\nhmm %s\nhyperGeom %s" % (planted, got, hyper), file=sys.stderr)


def _write_inputs(tmp_path, n, seed=1):
    from hic_genome_assembler_amd import synth
    lay, C = _map(n, seed)
    paths = synth.write_hicpro(str(tmp_path / "in"), lay, C)
    return paths


def _run_part1(paths, out, modularity, min_size=5):
    from hic_genome_assembler_amd import scaffoldToChromosomes as p1
    os.makedirs(out, exist_ok=True)
    f = lambda k: os.path.join(out, k)  # noqa: E731
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        p1.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                       paths["hicProScaffSizeFile"], f("dendrogramOrder.txt"), f("a.png"), f("b.png"), f("binGroups.txt"),
                       f("assessment.txt"), f("chromosomeGroups.txt"), False, True, min_size, modularity, 20, .05, 5, .2,
                       100000)
    return buf.getvalue(), f


def test_pipeline_with_hmm_at_2000_bins(tmp_path, monkeypatch, map2000):
    """runPipeline with HICMI_HMM=1: the six files (Part 1's four, Part 2's two from its chromosome groups), the HMM
    cuts those of the restatement, and two runs with the same HICMI_HMM_SEED byte-identical."""
    from hic_genome_assembler_amd import orderGenome as p2
    monkeypatch.setenv("HICMI_HMM", "1")
    monkeypatch.setenv("HICMI_HMM_SEED", "0")
    paths = _write_inputs(tmp_path, 2000)
    log1, f1 = _run_part1(paths, str(tmp_path / "r1"), .05)
    _log2, f2 = _run_part1(paths, str(tmp_path / "r2"), .05)
    names = ("dendrogramOrder.txt", "binGroups.txt", "assessment.txt", "chromosomeGroups.txt")
    for k in names:
        assert os.path.getsize(f1(k)) > 0
        assert open(f1(k)).read() == open(f2(k)).read(), k
    assert "Working on iterative 2 state HMMs" in log1
    _lay, _C, _leaves, A = map2000
    want = ref.identifyChromosomeGroupsHMM(ref.NumpyBackend(A, seed=0), 5, .05, 5, .2)
    cuts = eval(log1.split("CutIndices = ")[-1].splitlines()[0])
    assert cuts[:len(want)] == want                      # then the Louvain tail's cuts
    with contextlib.redirect_stdout(io.StringIO()):
        p2.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], f1("chromosomeGroups.txt"),
                       f1("chromosomeOrders.txt"), str(tmp_path / "r1"), "synthetic", f1("g.png"), "synthetic genome",
                       f1("plotOrder.txt"), 6, 5, 100000)
    for k in ("chromosomeOrders.txt", "plotOrder.txt"):
        assert os.path.getsize(f1(k)) > 0


def test_hmm_at_16000_bins(tmp_path, monkeypatch):
    """Part 1 with the HMM on the 16,000-bin map of bench.py (resident, modularity .05, the defaults): the four files,
    and a boundary at every planted chromosome boundary the hyperGeom path finds."""
    import torch
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as p1, synth
    from hic_genome_assembler_amd.hostio import Bin
    monkeypatch.setenv("HICMI_HMM", "1")
    n = 16000
    lay = synth.make_layout(n, seed=1)
    ct = synth.dense_contacts_torch(lay, torch.device("cuda", 0), seed=1, sinkhorn_iters=12)
    torch.cuda.synchronize()
    sizes = str(tmp_path / "sizes.txt")
    with open(sizes, "w") as fh:
        fh.write("".join("%s\t%d\n" % (nm, sz) for nm, sz in zip(lay.scaffold_names, lay.scaffold_sizes_bp)))
    bins = [Bin(int(lay.bin_ids[k]), lay.scaffold_names[lay.scaffold_of_bin[k]], int(lay.start[k]), int(lay.stop[k]),
                1.0, 0.0) for k in range(n)]
    names = ("dendrogramOrder.txt", "binGroups.txt", "assessment.txt", "chromosomeGroups.txt")
    fo = [str(tmp_path / k) for k in names]
    with _lib.Context(0) as ctx, contextlib.redirect_stdout(io.StringIO()):
        ctx.set_contacts_device(ct.data_ptr(), n, keepalive=ct)
        m = p1.DeviceMatrix(ctx)
        cuts = p1.runResident(m, bins, sizes, *fo, 5, .05, .05, hmm=True, convergenceRounds=5, lookAhead=.2)
        order = np.asarray(m.order)
    for k in fo:
        assert os.path.getsize(k) > 0
    chrom = lay.chrom_of_bin[order]
    planted = list(np.flatnonzero(np.diff(chrom)) + 1)
    assert len(cuts) >= len(planted) // 2
    hits = sum(1 for b in planted if min(abs(b - c) for c in cuts) <= 5)
    assert hits >= len(planted) - 2, (planted, cuts)
