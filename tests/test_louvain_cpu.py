"""CPU checks of the device Louvain path's host side (modularity.py, scaffoldToChromosomes.py):
* the PCG64 / random_interval / Fisher-Yates restatement k_louvain.hip follows equals numpy's Generator.permutation;
* the driver's split - level 0, then levels >= 1 from the generator state level 0 hands back - equals best_partition;
* the reference's stage functions logTransformMatrix and modularity_remaining_data;
* what the GPU edge tests rest on, on the host reference alone: the ties of the circulant graphs by lane, wave and stride,
  every pass gain clear of the threshold, the degenerate graphs' branches, the LDS rule against sizeof(LvShared), and the
  exact aggregation / score references against the host code."""
import contextlib
import io

import numpy as np
import pytest

import louvain_reference as lr
from hic_genome_assembler_amd import modularity as mod
from hic_genome_assembler_amd import scaffoldToChromosomes as p1


@pytest.mark.parametrize("size", [0, 1, 2, 3, 17, 800, 3200])
@pytest.mark.parametrize("seed,i", [(0, 0), (0, 7), (5, 1), (123456789, 19)])
def test_permutation_restatement_equals_numpy(size, seed, i):
    rng = np.random.default_rng([seed, i])
    rng.integers(0, 2 ** 31, size=1 + (i % 2), dtype=np.uint32)      # leave a buffered half behind on odd i
    pcg = lr.Pcg64(rng.bit_generator.state)
    assert np.array_equal(pcg.permutation(size), rng.permutation(size))
    present = np.flatnonzero(np.arange(size) % 3 != 1)                  # an int64 array, as _one_level shuffles
    assert np.array_equal(pcg.permutation(present), rng.permutation(present))
    assert pcg.state() == rng.bit_generator.state


def _graphs():
    return [("planted", lr.planted([30, 22, 14, 9], 3)), ("planted2", lr.planted([14, 9, 21, 6], 31)),
            ("n400_tail", lr.n400_tail()), ("quantised", lr.quantised(60, 4, 2))]


def _split_partition(A, seed, i):
    """What modularity_rounds_device does with the device calls replaced by host code."""
    st, rng, _passes = lr.host_level0(A, seed, i)
    part0 = mod._renumber(st.node2com)
    mod0 = mod._status_modularity(st.node2com, st.degrees, st.internals, st.total_weight)
    assert mod0 == st.modularity()
    return mod.upper_levels(mod._induced(A, part0), mod0, part0, rng)


@pytest.mark.parametrize("name,A", _graphs())
def test_split_equals_best_partition(name, A):
    for seed in (0, 3):
        for i in range(4):
            ref = mod.best_partition(A, np.random.default_rng([seed, i]))
            assert np.array_equal(_split_partition(A, seed, i), ref), (name, seed, i)


def test_quantised_graph_has_tied_moves():
    """The quantised graph makes moves whose best gain is tied (the device's shuffle replay path)."""
    A = lr.quantised(60, 4, 2)
    st = mod._Status(A.copy())
    rng = np.random.default_rng([0, 0])
    ties = [0]
    real_argmax = np.argmax

    def counting_argmax(v, *a, **k):
        v = np.asarray(v)
        if len(v) and np.max(v) > 0 and np.count_nonzero(v == np.max(v)) > 1:
            ties[0] += 1
        return real_argmax(v, *a, **k)
    mod.np.argmax = counting_argmax
    try:
        mod._one_level(st, rng)
    finally:
        mod.np.argmax = real_argmax
    assert ties[0] > 0


class _StageCtx:
    """The bits of a Context the Louvain tail reads on the host path: the similarity cells of the resident matrix."""

    def __init__(self, sim):
        self.sim = sim
        self.n = len(sim)

    def plot_downsample(self, kind, order, px):
        assert kind == 2 and px == len(order)
        o = np.asarray(order, dtype=np.int64)
        return self.sim[np.ix_(o, o)]


def _matrix(sim, order):
    m = p1.DeviceMatrix(_StageCtx(sim))
    m.order = list(order)
    return m


def test_log_transform_matrix_records_the_stage():
    m = _matrix(np.eye(3), range(3))
    with pytest.raises(ValueError):
        p1.logTransformMatrix(m)                       # contacts stage
    p1.convertMatrix(m, [], distance=False, similarity=True)
    assert p1.logTransformMatrix(m) is m and m.kind == "log-similarity"
    with pytest.raises(ValueError):
        p1.logTransformMatrix(m)                       # already log-transformed
    with pytest.raises(ValueError):
        p1.logTransformMatrix(m, reverse=True, logBase=2)
    p1.logTransformMatrix(m, reverse=True)
    assert m.kind == "similarity"
    with pytest.raises(ValueError):
        p1.logTransformMatrix(m, logBase=np.e)
    with pytest.raises(TypeError):
        p1.logTransformMatrix(np.eye(3))


def test_modularity_remaining_data_reference_signature(monkeypatch):
    """scaffoldToChromosomes.modularity_remaining_data(adjMat, binList, cutIndices, n_rounds) returns the reordered
    matrix and bins and the cut indices of runResident's tail branch (modularity.modularity_remaining_data on the
    log-transformed tail, then reorderMatrix)."""
    monkeypatch.delenv("HICMI_LOUVAIN_DEVICE", raising=False)
    rng = np.random.default_rng(4)
    n, head = 90, 40
    raw = np.abs(rng.normal(size=(n, n)))
    sim = raw + raw.T
    order = rng.permutation(n).tolist()
    bins = ["b%d" % i for i in range(n)]
    cuts = [12, head]
    with contextlib.redirect_stdout(io.StringIO()):
        tail = sim[np.ix_(order[head:], order[head:])]
        new_order, want_cuts = mod.modularity_remaining_data(mod.log_transform(tail), bins, cuts, n_rounds=3)
        m = _matrix(sim, order)
        with pytest.raises(ValueError):
            p1.modularity_remaining_data(m, bins, cuts, n_rounds=3)            # not at the log-similarity stage
        m.kind = "similarity"
        p1.logTransformMatrix(m)
        m2, bins2, cuts2 = p1.modularity_remaining_data(m, bins, cuts, n_rounds=3)
    assert m2 is m and cuts2 == want_cuts
    assert bins2 == [bins[i] for i in new_order]
    assert m.order == [order[i] for i in new_order]
    assert new_order[:head] == list(range(head))


# ---------------------------------------------------------------- conditions the GPU edge tests rest on
# (tests/test_gpu_louvain.py compares the device with these traces by `==` and leaves no case out; what makes that fair
# is asserted here, on the host reference alone)
def _case_names(prefix):
    return [n for n in lr.LEVEL0_CASES if n.startswith(prefix)]


def test_circulant_is_what_it_says():
    A = lr.circulant(600, lr.CIRCULANT_OFFSETS)
    assert np.array_equal(A, A.T) and not A.diagonal().any() and set(np.unique(A)) == {0.0, 1.0}
    assert np.array_equal(A.sum(axis=1), np.full(600, 6.0))
    assert np.flatnonzero(A[5]).tolist() == sorted((5 + s * o) % 600 for o in lr.CIRCULANT_OFFSETS for s in (1, -1))


@pytest.mark.parametrize("m", lr.CIRCULANT_M)
def test_circulant_ties_cross_lanes_waves_and_strides(m):
    """Every round has at least 100 tied moves, and tied ids in different waves, in different strides and in the same
    lane of two strides all occur; at m = 1030 the round's own partition has more than 256 communities."""
    A, states, traces = lr.level0_case("circulant-%d" % m)
    assert len(traces) == 2
    for i, t in enumerate(traces):
        cls, gains = lr.classify_ties(A, 0, i)
        assert cls == {"ties": t.ties, "cross_wave": t.cross_wave, "cross_stride": t.cross_stride, "same_lane": t.same_lane}
        assert gains == t.gains
        assert t.ties >= 100 and t.cross_wave > 0 and t.cross_stride > 0 and t.same_lane > 0, (m, i, cls)
        if m == 1030:
            assert len(np.unique(t.node2com)) > 256


@pytest.mark.parametrize("name", [n for n in lr.LEVEL0_CASES if n != "nan-cell"])
def test_pass_gains_stay_clear_of_the_threshold(name):
    """The device squares with x * x where NumPy calls pow(), so the two may stop after different passes when a gain is
    within an ulp or so of 1e-7 (the device counts gains within 1e-12 of it in info[2]).  Every gain of every case is
    1e-9 or more away - a thousand times that band - so passes compare by == and info[2] == 0 can be asserted."""
    _A, _states, traces = lr.level0_case(name)
    for t in traces:
        assert t.passes == len(t.gains) >= 1
        assert all(abs(g - 1e-7) >= 1e-9 for g in t.gains), (name, t.gains)


def test_thousand_rounds_tie_and_differ():
    _A, states, traces = lr.level0_case("rounds-1024")
    assert len(states) == len(traces) == lr.ROUNDS_MAX == 1024
    assert sum(t.ties for t in traces) > 0
    assert len({t.passes for t in traces}) > 1
    assert len({t.node2com.tobytes() for t in traces}) > 1


def test_buffered_entry_states_hold_a_half():
    for name in _case_names("buffered-"):
        _A, states, traces = lr.level0_case(name)
        for s, t in zip(states, traces):
            assert s["has_uint32"] == 1 and 0 < s["uinteger"] < 2 ** 32
            assert t.changed > 0
    assert sum(t.ties for t in lr.level0_case("buffered-circulant-300")[2]) > 0


def test_degenerate_graphs_do_what_the_gpu_tests_assume():
    # no link, and a NaN cell: links is 0 or NaN, every node's gains are NaN, nothing moves, one pass
    for name, m in (("zeros-5", 5), ("nan-cell", 75)):
        A, _states, traces = lr.level0_case(name)
        for t in traces:
            assert t.moves == t.nan_moves == m and t.passes == 1 and t.changed == 0 and t.ties == 0
            assert np.array_equal(t.node2com, np.arange(m))
    for t in lr.level0_case("zeros-5")[2]:
        assert t.gains == [0.0]                      # st.modularity() is 0.0 without links
    for t in lr.level0_case("nan-cell")[2]:
        # the gain is NaN on host and device: `NaN < 1e-7` is False, the loop ends on modified == False
        assert len(t.gains) == 1 and np.isnan(t.gains[0])
        assert np.isnan(t.degrees[[5, 9]]).all() and np.isfinite(np.delete(t.degrees, [5, 9])).all()
        assert np.isfinite(t.internals).all()
    with pytest.raises(ValueError, match="A graph without link"):
        with contextlib.redirect_stdout(io.StringIO()):
            mod.modularity_rounds(np.zeros((5, 5)), louvain_rounds=2, seed=0)
    # all ones: 257 communities stay 257 (a second stride of one community)
    for t in lr.level0_case("ones-257")[2]:
        assert t.changed == 0 and len(np.unique(t.node2com)) == 257 and t.nan_moves == 0 and t.passes == 1
    # isolated nodes stay alone, the rest moves; disconnected blocks come out as the blocks
    A = lr.isolated()
    assert not A[3].any() and not A[:, 17].any() and np.array_equal(A, A.T)
    for t in lr.level0_case("isolated")[2]:
        assert t.node2com[3] == 3 and t.node2com[17] == 17 and t.changed > 0
        assert np.count_nonzero(t.node2com == 3) == 1 and np.count_nonzero(t.node2com == 17) == 1
    A = lr.blocks()
    label = np.repeat(np.arange(5), (40, 25, 10, 1, 1))
    assert not A[label[:, None] != label[None, :]].any() and A[label[:, None] == label[None, :]].all()
    for t in lr.level0_case("blocks")[2]:
        assert np.array_equal(mod._renumber(t.node2com), label)
    for name in ("m3", "m3-pair", "stride-3"):
        assert len(lr.level0_case(name)[0]) == 3
    assert all(t.changed > 0 for t in lr.level0_case("m3-pair")[2])


@pytest.mark.parametrize("name", _case_names("stride-") + _case_names("slab-"))
def test_stride_and_slab_cases_move_nodes(name):
    A, states, traces = lr.level0_case(name)
    m = int(name.split("-")[1])
    assert len(A) == m and len(traces) == (4 if name.startswith("stride") else 3)
    if m > 3:
        assert all(t.changed >= m - 4 for t in traces)           # every node but one per group changes community


# ---- the LDS rule, restated: a round's arrays stay in LDS while
#      louvain_round_bytes(m) = 64 m <= louvain_level0_lds_max() = 160 KiB - sizeof(LvShared) - 1024
def _lvshared_size(tmp_path):
    """sizeof(LvShared) from a host-only compile of the struct as k_louvain.hip declares it (fixed-width integers and
    doubles only: the host and the device lay it out alike)."""
    import os
    import re
    import shutil
    import subprocess
    src = open(os.path.join(os.path.dirname(mod.__file__), "csrc", "k_louvain.hip")).read()
    struct = re.search(r"struct LvShared \{.*?\n\};", src, re.S).group(0)
    consts = "\n".join(re.findall(r"static constexpr int LV_(?:T|W) = [^;]*;", src))
    assert "LV_T" in consts and "LV_W" in consts
    prog = "#include <stdint.h>\n#include <stdio.h>\n%s\n%s\nint main() { printf(\"%%zu\\n\", sizeof(LvShared)); return 0; }\n"
    cpp = tmp_path / "lvshared.cpp"
    cpp.write_text(prog % (consts, struct))
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "lvshared"
    subprocess.check_call([cxx, "-std=c++17", "-o", str(exe), str(cpp)])
    return int(subprocess.check_output([str(exe)]).decode())


def test_lds_rule_boundary_sizes_straddle_it(tmp_path):
    import os
    csrc = os.path.join(os.path.dirname(mod.__file__), "csrc")
    assert lr.LDS_MAX_SRC in open(os.path.join(csrc, "k_louvain.hip")).read()
    assert lr.LDS_ROUND_BYTES_SRC in open(os.path.join(csrc, "hicmi_internal.h")).read()
    assert "louvain_round_bytes((int)m) <= (size_t)louvain_level0_lds_max()" in open(os.path.join(csrc, "api.hip")).read()
    lds_max = 160 * 1024 - _lvshared_size(tmp_path) - 1024
    assert lr.LDS_ROUND_BYTES == 64
    assert lr.LDS_ROUND_BYTES * lr.LDS_LAST_M <= lds_max < lr.LDS_ROUND_BYTES * lr.SLAB_FIRST_M
    assert lr.SLAB_FIRST_M == lr.LDS_LAST_M + 1
    assert lr.SLAB_M == (2400, lr.LDS_LAST_M, lr.SLAB_FIRST_M, 2600)


# ---------------------------------------------------------------- the exact references against the host code
def _induced_bound(part, k):
    """(2 |a| + |b|) 2^-53 per entry: see test_gpu_louvain.py (the sums are of non-negative terms)."""
    n = lr.induced_group_sizes(part, k).astype(np.float64)
    return (2.0 * n[:, None] + n[None, :]) * lr.EPS


@pytest.mark.parametrize("m", [1, 2, 255, 256, 257])
def test_exact_references_agree_with_the_host_code(m):
    for exact in (True, False):
        A = lr.agg_graph(m, exact)
        for k in lr.agg_ks(m):
            for name, part in lr.agg_partitions(m, k).items():
                want = lr.induced_fsum(A, part, k)
                if exact:
                    assert np.array_equal(want, lr.induced_exact(A, part, k)), (m, k, name)
                if len(np.unique(part)) == k:                         # _induced sizes its result by part.max()
                    got = mod._induced(A, part)
                    assert (np.abs(got - want) <= _induced_bound(part, k) * want).all(), (m, k, name)
                K = len(np.unique(part))
                q = lr.modularity_fsum(m - 1 - part, A)
                err = abs(np.longdouble(mod.modularity(m - 1 - part, A)) - q)
                assert err <= (m + 16) * K * lr.EPS, (m, k, name, float(err))
                if exact:
                    qe = lr.modularity_exact(m - 1 - part, A)
                    assert abs(float(q) - float(qe)) <= 2.0 ** -52, (m, k, name)
