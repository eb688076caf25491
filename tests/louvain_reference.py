"""Host restatements the Louvain tests compare the device against.

* numpy 2.2.6's Generator.permutation on PCG64: the 128-bit LCG, XSL-RR output, next_uint32 from the buffered halves of
  one 64-bit output (low half first), random_interval's mask-and-reject, Fisher-Yates from the top index down to 1.
  This is the draw sequence k_louvain.hip reproduces.
* test graphs: planted groups, quantised (tied) weights, and the n400_default fixture's log-similarity tail.
"""
import numpy as np

import golden_cases as gc

PCG_MULT = 0x2360ED051FC65DA44385DF649FCCF645
_M128 = (1 << 128) - 1
_M64 = (1 << 64) - 1


class Pcg64:
    """rng.bit_generator.state in, the same state out after the same draws."""

    def __init__(self, state):
        self.s = int(state["state"]["state"])
        self.inc = int(state["state"]["inc"])
        self.has = int(state["has_uint32"])
        self.uinteger = int(state["uinteger"])

    def state(self):
        return {"bit_generator": "PCG64", "state": {"state": self.s, "inc": self.inc},
                "has_uint32": self.has, "uinteger": self.uinteger}

    def next64(self):
        self.s = (self.s * PCG_MULT + self.inc) & _M128
        hi, lo = self.s >> 64, self.s & _M64
        rot = hi >> 58
        x = hi ^ lo
        return ((x >> rot) | (x << ((64 - rot) & 63))) & _M64

    def next32(self):
        if self.has:
            self.has = 0
            return self.uinteger
        v = self.next64()
        self.has, self.uinteger = 1, v >> 32
        return v & 0xFFFFFFFF

    def interval(self, mx):
        if mx == 0:
            return 0
        mask = mx
        for sh in (1, 2, 4, 8, 16, 32):
            mask |= mask >> sh
        while True:
            v = self.next32() & mask
            if v <= mx:
                return v

    def permutation(self, x):
        arr = np.arange(x) if isinstance(x, (int, np.integer)) else np.array(x)
        for i in range(len(arr) - 1, 0, -1):
            j = self.interval(i)
            arr[i], arr[j] = arr[j], arr[i]
        return arr


# ---------------------------------------------------------------- graphs
def planted(sizes, seed, strong=3.0, weak=0.05):
    """Symmetric weights with planted groups (the graph the host builds is graph_weights of it)."""
    from hic_genome_assembler_amd import modularity as mod
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    label = np.repeat(np.arange(len(sizes)), sizes)
    a = rng.random((n, n)) * weak
    same = label[:, None] == label[None, :]
    a[same] += strong * (0.5 + rng.random(int(same.sum())))
    return mod.graph_weights(a)


def quantised(n, groups, seed):
    """Weights on a coarse grid (0.5, 1, 2): many equal gains, so moves with tied best gains are frequent."""
    from hic_genome_assembler_amd import modularity as mod
    rng = np.random.default_rng(seed)
    label = rng.integers(0, groups, n)
    a = np.where(label[:, None] == label[None, :], 2.0, 0.5)
    a = np.where(rng.random((n, n)) < 0.3, 1.0, a)
    return mod.graph_weights(a)


def n400_tail():
    """The log-similarity tail (last 13 %) of the n400_default fixture in its dendrogram order, and the graph."""
    import hic_oracle as orc
    from hic_genome_assembler_amd import modularity as mod
    spec, meta, gold, lay, c = gc.load_case("n400_default")
    dist = orc.to_distance(c)
    leaves, _z = orc.average_cluster_leaves(dist)
    bins = [orc.Bin(i, "s", 0, 0, 0.0, 0.0) for i in range(len(c))]
    _m, bins = orc.remove_zero_rows(c.copy(), bins)
    sim = orc.to_similarity(dist[:, leaves][leaves], [bins[i] for i in leaves])
    start = int(len(c) * 0.87)
    return mod.graph_weights(mod.log_transform(sim)[start:, start:])


def host_level0(A, seed, i):
    """_one_level(_Status(A.copy()), default_rng([seed, i])): (status, rng, passes)."""
    from hic_genome_assembler_amd import modularity as mod
    rng = np.random.default_rng([seed, i])
    st = mod._Status(np.array(A, dtype=np.float64))
    passes = [0]
    real = rng.permutation

    class Counting:                      # counts the passes: one permutation(n) per pass
        def __getattr__(self, k):
            return getattr(rng, k)

        def permutation(self, x):
            if isinstance(x, (int, np.integer)):
                passes[0] += 1
            return real(x)
    mod._one_level(st, Counting())
    return st, rng, passes[0]
