"""The Louvain tail (modularity > 0, S2C:239-349) on the GPU with HICMI_LOUVAIN_DEVICE=1: the graph build against the
host's graph_weights(log_transform(...)), level 0 bit for bit against modularity._one_level (partition, passes, PCG64
state, tie replays) at the kernel's wave, stride, slab, round-count and data edges, the aggregation and score against
exact and correctly rounded references within derived bounds, the best of rounds against modularity_rounds, and Part 1's
files with and without the switch."""
import contextlib
import io
import os
import sys

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


# ---------------------------------------------------------------- level 0 at the kernel's edges
# Every case is a graph and a list of generator states (tests/louvain_reference.py); all its rounds run in ONE launch and
# each is compared with the host's traced _one_level.  tests/test_louvain_cpu.py asserts, on the host alone, what makes
# `==` fair: no pass gain within 1e-9 of the 1e-7 threshold, and the ties / strides / slab sizes each case is there for.
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check_case(ctx, name):
    A, states, traces = lr.level0_case(name)
    ctx.louvain_set_graph(A)
    n2c, out, info, deg, inr = ctx.louvain_level0(states)
    for i, t in enumerate(traces):
        print("level0 %-22s m %4d round %4d  passes host %2d device %2d  ties host %4d device %4d  (cross-wave %d, "
              "cross-stride %d, same-lane %d)" % (name, len(A), i, t.passes, info[i, 0], t.ties, info[i, 1], t.cross_wave,
                                                  t.cross_stride, t.same_lane), file=sys.stderr)
    for i, t in enumerate(traces):
        assert np.array_equal(n2c[i], t.node2com), (name, i)
        assert info[i, 0] == t.passes, (name, i)
        assert out[i] == t.state, (name, i)
        # by bit pattern, so that NaN equals NaN and -0.0 is not 0.0
        assert np.array_equal(_bits(deg[i]), _bits(t.degrees)), (name, i)
        assert np.array_equal(_bits(inr[i]), _bits(t.internals)), (name, i)
        assert info[i, 1] == t.ties, (name, i)            # the shuffle replay ran exactly as often as the host tied
        assert info[i, 2] == 0 and info[i, 3] == 0, (name, i)
    return traces


@pytest.mark.parametrize("m", lr.CIRCULANT_M)
def test_level0_ties_across_lanes_waves_and_strides(ctx, m):
    """circulant(m, (1, 64, 256)): hundreds of moves per round whose best gain is reached by communities in other lanes,
    other waves and the same lane of another stride of the argmax; m = 1030 keeps more than 256 communities."""
    traces = _check_case(ctx, "circulant-%d" % m)
    assert all(t.ties >= 100 and t.cross_wave and t.cross_stride and t.same_lane for t in traces)


@pytest.mark.parametrize("m", lr.SLAB_M)
def test_level0_either_side_of_the_lds_limit(ctx, m):
    """2508 is the largest m whose round state fits in LDS and 2509 the first that runs from the global slab, where
    rounds 1 and 2 start at scratch + r * 64 m; 2400 and 2600 lie safely on either side."""
    _check_case(ctx, "slab-%d" % m)


@pytest.mark.parametrize("m", lr.STRIDE_M)
def test_level0_loop_strides(ctx, m):
    """m around 64, 256, 512 and 1024: the community loops run one, two, three and five trips, waves 1 to 3 hold
    communities or none, and the member rotation after a move spans more than one trip."""
    _check_case(ctx, "stride-%d" % m)


def test_level0_1024_rounds_in_one_launch(ctx):
    traces = _check_case(ctx, "rounds-1024")
    assert len(traces) == 1024


@pytest.mark.parametrize("name", ["buffered-planted", "buffered-circulant-300"])
def test_level0_entry_state_with_a_buffered_half(ctx, name):
    """The generator comes in with has_uint32 = 1: the first draw is the waiting `uinteger`, not a new output."""
    _check_case(ctx, name)


@pytest.mark.parametrize("name", ["zeros-5", "ones-257", "isolated", "blocks", "nan-cell", "m3", "m3-pair"])
def test_level0_degenerate_data(ctx, name):
    """No link at all (links = 0, every gain NaN), all ones (nothing moves, 257 communities), isolated nodes, blocks with
    exact zeros between them, a NaN cell (links = NaN) and three nodes."""
    _check_case(ctx, name)


def test_graph_without_link_raises_as_on_the_host(ctx):
    from hic_genome_assembler_amd import modularity as mod
    A = np.zeros((5, 5))
    with contextlib.redirect_stdout(io.StringIO()):
        with pytest.raises(ValueError) as host:
            mod.modularity_rounds(A, louvain_rounds=2, seed=0)
        ctx.louvain_set_graph(A)
        with pytest.raises(ValueError) as dev:
            mod.modularity_rounds_device(ctx, louvain_rounds=2, seed=0)
    assert str(dev.value) == str(host.value) == "A graph without link has an undefined modularity"
    # The NaN graph is compared at level 0 only (test_level0_degenerate_data).  Above it the two wrappers fail in
    # different ways on an input that cannot occur - log10(similarity + 1) of finite contacts is finite - so neither
    # failure is pinned.


# ---------------------------------------------------------------- aggregation and score
# u = 2^-53.
#
# Aggregated graph, B[a][b] with |a| and |b| members.  The device sums non-negative terms in two sequential stages:
# rowagg[i][b] over the |b| members of b from 0.0 (the first add is exact: <= (|b| - 1) u relative), then over the |a|
# members of a (<= (|a| - 1) u more).  The diagonal adds the members' self loops, a sum of |a| terms ((|a| - 1) u on a
# part of the total), in one more rounding, and halves exactly.  With the reference's own rounding (math.fsum: u) that
# is <= (|a| + |b|) u, within the (2 |a| + |b|) u asserted; an empty community gives exactly 0 on both sides.  On
# integer weights every partial sum is an integer below 2^53: the result is exact and compared bit for bit.
#
# Score on integer weights.  inc_c, deg_c and links reach k_lv_score exact.  Per community present:
#   t = (inc / 2) / links      one rounding, 0 <= t <= 1                                         u
#   a = deg / (2 links)        one rounding, 0 <= a <= 1: its error doubles in a * a           2 u
#   s = a * a                  one rounding, s <= 1                                              u
#   d = t - s                  one rounding, |d| <= 1                                            u
#   res += d                   one rounding; every partial sum is sum t - sum s, both in [0, 1]   u
# six roundings of values at most 1: |Q_device - Q| <= 6 K u with K communities present (to first order in u).
#
# Score on rounded weights, against the longdouble value: now inc_c, deg_c and links are rounded sums of up to m terms.
# No allowance may exceed (m + 16) K u - per community m u for sums of up to m terms had they been added one after the
# other, and 16 u for the operations above on inputs that carry an error already.  The device's sums are pairwise or
# tree-shaped and land far below that: SCORE_ALLOW is 8 times the largest error measured over all cases of
# test_induced_and_score_on_rounded_weights and test_induced_and_modularity on an MI355X, rounded up to a power of two
# (DESIGN.md section 9b has the figures), and the smaller of the two is asserted.
U = lr.EPS
SCORE_ALLOW = 2.0 ** -47         # measured: 5.996 u (m = 1000, one community); 8 x 5.996 u = 47.97 u -> 64 u


def _induced_bound(part, k):
    n = lr.induced_group_sizes(part, k).astype(np.float64)
    return (2.0 * n[:, None] + n[None, :]) * U


def _score_allow(m, K):
    return min(SCORE_ALLOW, (m + 16) * K * U)


def _check_induced_rounded(ctx, A, part, k, what):
    assert (A >= 0).all()
    B = ctx.louvain_induced(part, k)
    want = lr.induced_fsum(A, part, k)
    err = np.abs(B - want)
    bound = _induced_bound(part, k) * want
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(want > 0, err / (want * U), 0.0)))
    print("induced %s  worst error %.3g u relative (allowed per entry: 2 |a| + |b|)" % (what, worst), file=sys.stderr)
    assert (err <= bound).all(), what


def _check_score_rounded(ctx, A, parts, what):
    """parts: a list of label vectors, scored in ONE call; returns the largest error in units of u."""
    m = len(A)
    q = ctx.louvain_modularity(np.stack(parts))
    worst = 0.0
    for p, qq in zip(parts, q):
        K = len(np.unique(p))
        err = float(abs(np.longdouble(qq) - lr.modularity_fsum(p, A)))
        print("score-rounded %s m %4d K %4d  error %.4g u  (allowed %.4g u)" % (what, m, K, err / U, _score_allow(m, K) / U),
              file=sys.stderr)
        assert err <= _score_allow(m, K), (what, K, err / U)
        worst = max(worst, err / U)
    return worst


_AGG_CASES = [(m, k) for m in lr.AGG_M for k in lr.agg_ks(m)]


@pytest.mark.parametrize("m,k", _AGG_CASES)
def test_induced_and_score_on_integer_weights(ctx, m, k):
    """Weights 0..7: louvain_induced equals the integer sums bit for bit; louvain_modularity is within 6 K u of the
    Fraction value, five partitions in one call and one at a time under reversed, non-contiguous labels."""
    from fractions import Fraction
    A = lr.agg_graph(m, True)
    ctx.louvain_set_graph(A)
    parts = lr.agg_partitions(m, k)
    exact = {}
    for name, part in parts.items():
        B = ctx.louvain_induced(part, k)
        assert np.array_equal(_bits(B), _bits(lr.induced_exact(A, part, k))), (m, k, name)
        exact[name] = lr.modularity_exact(part, A)
    names = list(parts)[:5]
    runs = [("R5", n, q) for n, q in zip(names, ctx.louvain_modularity(np.stack([parts[n] for n in names])))]
    runs += [("R1", n, ctx.louvain_modularity(m - 1 - p[None, :])[0]) for n, p in parts.items()]
    for how, name, q in runs:
        K = len(np.unique(parts[name]))
        err = abs(Fraction(float(q)) - exact[name])
        print("score-exact %s m %4d k %4d %-8s K %4d  error %.4g u  (allowed %d u)" % (how, m, k, name, K, float(err / Fraction(U)),
                                                                                    6 * K), file=sys.stderr)
        assert err <= 6 * K * Fraction(U), (how, m, k, name)


def test_score_of_1024_partitions_on_integer_weights(ctx):
    """R = 1024 at m = 24 in one call: every round reads its own partition and writes its own accumulators."""
    from fractions import Fraction
    m = 24
    A = lr.agg_graph(m, True)
    ctx.louvain_set_graph(A)
    rng = np.random.default_rng(47)
    parts = np.stack([rng.integers(0, 1 + r % m, m) if r % 2 else m - 1 - rng.integers(0, 1 + r % m, m) for r in range(1024)])
    assert len({p.tobytes() for p in parts}) > 900
    q = ctx.louvain_modularity(parts)
    worst = 0.0
    for p, qq in zip(parts, q):
        err = abs(Fraction(float(qq)) - lr.modularity_exact(p, A))
        assert err <= 6 * len(np.unique(p)) * Fraction(U)
        worst = max(worst, float(err / Fraction(U)))
    print("score-exact R1024 m 24  worst error %.4g u" % worst, file=sys.stderr)


@pytest.mark.parametrize("m,k", _AGG_CASES)
def test_induced_and_score_on_rounded_weights(ctx, m, k):
    """rng.random weights: louvain_induced within (2 |a| + |b|) u relative of math.fsum per entry, louvain_modularity
    within SCORE_ALLOW (and never more than (m + 16) K u) of the longdouble value."""
    A = lr.agg_graph(m, False)
    ctx.louvain_set_graph(A)
    parts = lr.agg_partitions(m, k)
    for name, part in parts.items():
        if name != "random2":
            _check_induced_rounded(ctx, A, part, k, "m %4d k %4d %-8s" % (m, k, name))
    names = list(parts)[:5]
    _check_score_rounded(ctx, A, [parts[n] for n in names], "R5 k %4d" % k)
    for name, part in parts.items():
        _check_score_rounded(ctx, A, [m - 1 - part], "R1 k %4d %-8s" % (k, name))


def test_induced_and_modularity(ctx):
    from hic_genome_assembler_amd import modularity as mod
    for name, A in _graphs().items():
        ctx.louvain_set_graph(A)
        rng = np.random.default_rng(5)
        parts = []
        for k in (1, 3, 7):
            part = mod._renumber(rng.integers(0, k, len(A)))
            kk = int(part.max()) + 1
            _check_induced_rounded(ctx, A, part, kk, "%-9s k %d" % (name, kk))
            parts.append(part)
        _check_score_rounded(ctx, A, parts, name)


def test_best_of_rounds_equals_host(ctx):
    from hic_genome_assembler_amd import modularity as mod
    # (the circulant graph: a flow with hundreds of tied moves and a hundred communities at level 0)
    for name, A in list(_graphs().items()) + [("circulant-300", lr.circulant(300, lr.CIRCULANT_OFFSETS))]:
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
            c.louvain_level0(st * 1025)                    # too many rounds (1024 run in test_level0_1024_rounds_in_one_launch)
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
