"""The Louvain tail (modularity > 0, S2C:239-349) on the GPU with HICMI_LOUVAIN_DEVICE=1: the graph build against the
host's graph_weights(log_transform(...)), level 0 bit for bit against modularity._one_level (partition, passes, PCG64
state), the aggregation and score within 1e-12, the best of rounds against modularity_rounds, and Part 1's files with
and without the switch."""
import contextlib
import io
import os

import numpy as np
import pytest

import golden_cases as gc
import hmm_reference as href
import louvain_reference as lr

pytestmark = pytest.mark.gpu


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


@pytest.fixture(scope="module")
def ctx():
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as c:
        yield c


def _graphs():
    return {"planted": lr.planted([30, 22, 14, 9], 3), "planted2": lr.planted([14, 9, 21, 6], 31),
            "n400_tail": lr.n400_tail(), "quantised": lr.quantised(60, 4, 2), "m1": np.array([[0.7]]),
            "m2": np.array([[0.2, 1.5], [1.5, 0.0]])}


# ---------------------------------------------------------------- graph build
def test_graph_build_n400_tail(ctx):
    from hic_genome_assembler_amd import modularity as mod
    spec, meta, gold, lay, C = gc.load_case("n400_default")
    ctx.set_contacts(C)
    ctx.row_sums()
    leaves, _z = ctx.upgma(want_linkage=False)
    leaves = np.asarray(leaves)
    start = int(len(C) * 0.87)
    ctx.louvain_graph(leaves[start:])
    A, gdeg, total = ctx.louvain_get_graph()
    want = mod.graph_weights(href.log_similarity(C, leaves)[start:, start:])
    assert int(_ulps(A, want).max()) <= 2
    assert np.array_equal(A, A.T)
    st = mod._Status(A.copy())
    assert total == st.total_weight and np.array_equal(gdeg, st.gdegrees)


def test_graph_build_bench_map_tail(ctx):
    """The 16,000-bin map of bench.py: the last 5 % of its dendrogram order (m = 800)."""
    import torch
    from hic_genome_assembler_amd import _lib, modularity as mod, synth
    n = 16000
    lay = synth.make_layout(n, seed=1)
    ct = synth.dense_contacts_torch(lay, torch.device("cuda", 0), seed=1, sinkhorn_iters=12)
    torch.cuda.synchronize()
    with _lib.Context(0) as c16:
        c16.set_contacts_device(ct.data_ptr(), n, keepalive=ct)
        np_sum, seq_sum = c16.row_sums()
        leaves, _z = c16.upgma(want_linkage=False)
        rows = np.asarray(leaves)[n - 800:]
        c16.louvain_graph(rows)
        A, gdeg, total = c16.louvain_get_graph()
    r = torch.as_tensor(rows.astype(np.int64), device=ct.device)
    Ct = ct[r][:, r].double().cpu().numpy()
    d = (1.0 - (Ct / np.asarray(np_sum)[rows][:, None])) + 1.0
    s = np.asarray(seq_sum)[rows][:, None] * (1.0 - (d - 1.0))
    want = mod.graph_weights(mod.log_transform(s))
    assert int(_ulps(A, want).max()) <= 2
    assert np.array_equal(A, A.T)
    st = mod._Status(A.copy())
    assert total == st.total_weight and np.array_equal(gdeg, st.gdegrees)


# ---------------------------------------------------------------- level 0
def _check_level0(ctx, A, seeds, rounds):
    ctx.louvain_set_graph(A)
    ties = 0
    for seed in seeds:
        states = [np.random.default_rng([seed, i]).bit_generator.state for i in range(rounds)]
        n2c, out, info, deg, inr = ctx.louvain_level0(states)
        for i in range(rounds):
            st, rng, passes = lr.host_level0(A, seed, i)
            assert np.array_equal(n2c[i], st.node2com), (seed, i)
            assert info[i, 0] == passes, (seed, i)
            assert out[i] == rng.bit_generator.state, (seed, i)
            assert np.array_equal(deg[i], st.degrees) and np.array_equal(inr[i], st.internals), (seed, i)
            assert info[i, 2] == 0
        ties += int(info[:, 1].sum())
    return ties


@pytest.mark.parametrize("name", ["planted", "planted2", "n400_tail", "quantised", "m1", "m2"])
def test_level0_bit_identical(ctx, name):
    ties = _check_level0(ctx, _graphs()[name], seeds=(0, 3), rounds=4)
    if name == "quantised":
        assert ties > 0                                   # the shuffle replay ran


def test_level0_bit_identical_at_3200(ctx):
    A = lr.planted([400] * 8, 11)
    _check_level0(ctx, A, seeds=(0,), rounds=1)


def test_induced_and_modularity(ctx):
    from hic_genome_assembler_amd import modularity as mod
    for name, A in _graphs().items():
        ctx.louvain_set_graph(A)
        rng = np.random.default_rng(5)
        parts = []
        for k in (1, 3, 7):
            part = mod._renumber(rng.integers(0, k, len(A)))
            kk = int(part.max()) + 1
            B = ctx.louvain_induced(part, kk)
            want = mod._induced(A, part)
            assert np.allclose(B, want, rtol=1e-12, atol=0), name
            parts.append(part)
        q = ctx.louvain_modularity(np.stack(parts))
        for p, qq in zip(parts, q):
            want = mod.modularity(p, A)
            assert abs(qq - want) <= 1e-12 * max(1.0, abs(want)), name


def test_best_of_rounds_equals_host(ctx):
    from hic_genome_assembler_amd import modularity as mod
    for name, A in _graphs().items():
        if name == "m1":
            continue
        with contextlib.redirect_stdout(io.StringIO()) as host_log:
            want, want_q = mod.modularity_rounds(A, louvain_rounds=5, seed=2)
        ctx.louvain_set_graph(A)
        runs = []
        for _ in range(2):
            with contextlib.redirect_stdout(io.StringIO()) as dev_log:
                got, got_q = mod.modularity_rounds_device(ctx, louvain_rounds=5, seed=2)
            runs.append((got.tobytes(), got_q, dev_log.getvalue()))
        assert np.array_equal(got, want), name
        assert abs(got_q - want_q) <= 1e-12, name
        assert runs[0] == runs[1]                          # byte-identical repeats
        assert dev_log.getvalue().count("Louvain round") == host_log.getvalue().count("Louvain round")


def test_level0_misuse_is_reported(ctx):
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as c:
        st = [np.random.default_rng(0).bit_generator.state]
        with pytest.raises(_lib.HicmiError):
            c.louvain_level0(st)                           # no graph
        with pytest.raises(_lib.HicmiError):
            c.louvain_set_graph(np.zeros((0, 0)))          # m = 0
        with pytest.raises(_lib.HicmiError):
            c.louvain_graph([0, 1])                        # no contact matrix
        c.louvain_set_graph(np.ones((3, 3)))
        with pytest.raises(_lib.HicmiError):
            c.louvain_level0(st * 1025)                    # too many rounds
        with pytest.raises(_lib.HicmiError):
            c.louvain_induced(np.array([0, 1, 2, 3]), 4)   # wrong m
        with pytest.raises(_lib.HicmiError):
            c.louvain_modularity(np.zeros((1, 5), np.int32))


def test_graph_above_the_supported_size_is_refused(ctx):
    """m > 16,384 comes back as HICMI_EUNSUPPORTED before anything is allocated or launched."""
    from hic_genome_assembler_amd import _lib
    lib = _lib.load()
    HICMI_EUNSUPPORTED = -5
    assert lib.hicmi_louvain_set_graph(ctx._h, None, 16385) == HICMI_EUNSUPPORTED
    rows = np.zeros(16385, np.int32)
    assert lib.hicmi_louvain_graph(ctx._h, rows.ctypes.data_as(_lib._vp), 16385) == HICMI_EUNSUPPORTED


# ---------------------------------------------------------------- Part 1 with and without the switch
def _part1(paths, out, modularity, hmm=False, rounds=20, min_size=5, psig=.05, resolution=100000):
    from hic_genome_assembler_amd import scaffoldToChromosomes as p1
    os.makedirs(out, exist_ok=True)
    f = lambda k: os.path.join(out, k)  # noqa: E731
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        p1.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                       paths["hicProScaffSizeFile"], f("dendrogramOrder.txt"), False, False, f("binGroups.txt"),
                       f("assessment.txt"), f("chromosomeGroups.txt"), not hmm, hmm, min_size, modularity, rounds,
                       psig, 5, .2, resolution)
    return {k: open(f(k)).read() for k in ("binGroups.txt", "assessment.txt", "chromosomeGroups.txt")}, buf.getvalue()


def _same_with_and_without(tmp_path, monkeypatch, paths, **kw):
    monkeypatch.delenv("HICMI_LOUVAIN_DEVICE", raising=False)
    host, host_log = _part1(paths, str(tmp_path / "host"), .05, **kw)
    monkeypatch.setenv("HICMI_LOUVAIN_DEVICE", "1")
    dev, dev_log = _part1(paths, str(tmp_path / "dev"), .05, **kw)
    assert "Maximizing so-called modularity" in host_log and "Maximizing so-called modularity" in dev_log
    for k in host:
        assert dev[k] == host[k], k


@pytest.mark.parametrize("name", ["n400_default", "n2000"])
def test_pipeline_files_equal_with_and_without_the_switch(tmp_path, monkeypatch, name):
    spec, meta, gold, lay, c = gc.load_case(name)
    paths = gc.write_case_files(name, str(tmp_path))
    _same_with_and_without(tmp_path, monkeypatch, paths, min_size=spec["min_size"], psig=spec["psig"],
                           resolution=lay.resolution)


def test_pipeline_hmm_files_equal_with_and_without_the_switch(tmp_path, monkeypatch):
    from hic_genome_assembler_amd import synth
    monkeypatch.setenv("HICMI_HMM", "1")
    lay = synth.make_layout(2000, seed=1)
    C = synth.dense_contacts(lay, seed=1)
    paths = synth.write_hicpro(str(tmp_path / "in"), lay, C)
    _same_with_and_without(tmp_path, monkeypatch, paths, hmm=True)


def test_modularity_alone_on_4000_bins(ctx, monkeypatch):
    """No cut found (cutIndices = []): the whole map is partitioned; the device partition equals the host's."""
    from hic_genome_assembler_amd import modularity as mod, synth
    lay = synth.make_layout(4000, seed=3)
    C = synth.dense_contacts(lay, seed=3)
    ctx.set_contacts(C)
    ctx.row_sums()
    leaves, _z = ctx.upgma(want_linkage=False)
    bins = list(range(4000))
    ctx.louvain_graph(np.asarray(leaves))
    A, _g, _t = ctx.louvain_get_graph()
    with contextlib.redirect_stdout(io.StringIO()):
        dev = mod.modularity_remaining_data(None, bins, [], n_rounds=1, ctx=ctx)
    with contextlib.redirect_stdout(io.StringIO()):
        host = mod.modularity_remaining_data(A, bins, [], n_rounds=1)
    assert dev == host
