"""CPU checks of the device Louvain path's host side (modularity.py, scaffoldToChromosomes.py):
* the PCG64 / random_interval / Fisher-Yates restatement k_louvain.hip follows equals numpy's Generator.permutation;
* the driver's split - level 0, then levels >= 1 from the generator state level 0 hands back - equals best_partition;
* the reference's stage functions logTransformMatrix and modularity_remaining_data."""
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
