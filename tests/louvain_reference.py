"""Host restatements the Louvain tests compare the device against.

* numpy 2.2.6's Generator.permutation on PCG64: the 128-bit LCG, XSL-RR output, next_uint32 from the buffered halves of
  one 64-bit output (low half first), random_interval's mask-and-reject, Fisher-Yates from the top index down to 1.
  This is the draw sequence k_louvain.hip reproduces.
* test graphs: planted groups, quantised (tied) weights, and the n400_default fixture's log-similarity tail;
* the graphs, generator states and traced host runs of the level-0 edge cases (ties across lanes, waves and strides, the
  LDS limit, loop strides, 1,024 rounds, a buffered entry state, degenerate data);
* the community graph and the modularity score from their definitions: in integers / Fractions and with math.fsum / longdouble.
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


# ---------------------------------------------------------------- graphs for the wave, stride and slab edges
def circulant(m, offsets):
    """0/1 symmetric: A[i][(i +- o) % m] = 1 for every offset, zero diagonal, zero elsewhere.  Every node has the same
    degree, so a node's neighbours offer equal gains: with offsets (1, 64, 256) the tied communities of a move sit in
    another lane (+-1), another wave (+-64) and the same lane of another stride (+-256) of the 256-thread argmax."""
    a = np.zeros((m, m))
    i = np.arange(m)
    for o in offsets:
        a[i, (i + o) % m] = 1.0
        a[i, (i - o) % m] = 1.0
    a[i, i] = 0.0
    return a


def four_groups(m, seed):
    """planted groups of sizes m // 4 (three times) and the rest."""
    q = m // 4
    return planted([q, q, q, m - 3 * q], seed)


def isolated():
    """planted([30, 22, 14, 9], 3) with nodes 3 and 17 cut off: their rows and columns (self loops too) are zero."""
    a = planted([30, 22, 14, 9], 3)
    for i in (3, 17):
        a[i, :] = 0.0
        a[:, i] = 0.0
    return a


def nan_cell():
    """The isolated-nodes graph with one NaN edge: every sum over the matrix, hence every gain, is NaN."""
    a = isolated()
    a[5, 9] = a[9, 5] = np.nan
    return a


def blocks(sizes=(40, 25, 10, 1, 1), seed=7):
    """Planted diagonal blocks with exact zeros between them (two of the blocks are a lone node with a self loop)."""
    a = planted(list(sizes), seed)
    label = np.repeat(np.arange(len(sizes)), sizes)
    a[label[:, None] != label[None, :]] = 0.0
    return a


def buffered_state(seed, i):
    """default_rng([seed, i]) after one uint32 draw: has_uint32 = 1 and the other half of the 64-bit output waiting in
    `uinteger` - the state a generator is in when Louvain is not its first user."""
    rng = np.random.default_rng([seed, i])
    rng.integers(0, 2 ** 31, size=1, dtype=np.uint32)
    st = rng.bit_generator.state
    assert st["has_uint32"] == 1 and st["uinteger"] != 0
    return st


# ---------------------------------------------------------------- level 0 on the host, traced
class Level0:
    """What _one_level left behind and what it did on the way (one round)."""

    def __init__(self):
        self.node2com = self.degrees = self.internals = self.state = None
        self.passes = 0
        self.gains = []            # new_mod - cur_mod of every pass
        self.moves = 0             # argmax calls (node visits with a community present)
        self.nan_moves = 0         # of them, with a NaN gain (np.argmax stops there and `> 0` fails)
        self.ties = 0              # max > 0 reached more than once: the device must replay the shuffle
        self.cross_wave = 0        # ... by ids with different (c % 256) // 64
        self.cross_stride = 0      # ... by ids with different c // 256
        self.same_lane = 0         # ... by ids of which two share c % 256
        self.changed = 0           # nodes not in their own community at the end


class _NumpyWithArgmax:
    """numpy for modularity._one_level with argmax routed through a hook (numpy itself stays as it is)."""

    def __init__(self, hook):
        self.argmax = hook

    def __getattr__(self, k):
        return getattr(np, k)


def trace_level0(A, state):
    """modularity._one_level(_Status(A.copy()), rng) from the generator state `state`, recording `order` and `incr` of
    every move.  Returns a Level0."""
    from hic_genome_assembler_amd import modularity as mod
    rng = np.random.default_rng()
    rng.bit_generator.state = state
    st = mod._Status(np.array(A, dtype=np.float64))
    out = Level0()
    last = {}

    class Rng:                           # one permutation(n) per pass, one permutation(present) per node
        def __getattr__(self, k):
            return getattr(rng, k)

        def permutation(self, x):
            res = rng.permutation(x)
            if isinstance(x, (int, np.integer)):
                out.passes += 1
            else:
                last["order"] = res
            return res

    def argmax(incr, *a, **k):
        incr = np.asarray(incr)
        order = last["order"]
        assert len(order) == len(incr)
        out.moves += 1
        mx = np.max(incr)
        if mx != mx:
            out.nan_moves += 1
        elif mx > 0:
            tied = order[incr == mx]
            if len(tied) > 1:
                out.ties += 1
                out.cross_wave += len(set(((tied % 256) // 64).tolist())) > 1
                out.cross_stride += len(set((tied // 256).tolist())) > 1
                out.same_lane += len(set((tied % 256).tolist())) < len(tied)
        return np.argmax(incr, *a, **k)

    mods = []
    real_modularity = st.modularity

    def modularity():
        mods.append(real_modularity())
        return mods[-1]
    st.modularity = modularity
    saved = mod.np
    mod.np = _NumpyWithArgmax(argmax)
    try:
        with np.errstate(invalid="ignore", divide="ignore"):
            mod._one_level(st, Rng())
    finally:
        mod.np = saved
    out.gains = [b - a for a, b in zip(mods, mods[1:])]
    assert len(out.gains) == out.passes
    out.node2com, out.degrees, out.internals = st.node2com, st.degrees, st.internals
    out.state = rng.bit_generator.state
    out.changed = int(np.count_nonzero(st.node2com != np.arange(len(st.node2com))))
    return out


def classify_ties(A, seed, i):
    """_one_level on the host for round (seed, i): the counts of tied moves by where the tied ids sit in the device's
    256-thread argmax (total, cross-wave, cross-stride, same-lane) and the pass gains."""
    t = trace_level0(A, np.random.default_rng([seed, i]).bit_generator.state)
    return {"ties": t.ties, "cross_wave": t.cross_wave, "cross_stride": t.cross_stride, "same_lane": t.same_lane}, t.gains


# The level-0 cases of the edge tests: name -> (graph, [generator state per round]).  The graphs and their traces are
# computed once per process and never written to.
CIRCULANT_OFFSETS = (1, 64, 256)
CIRCULANT_M = (300, 600, 1030)
STRIDE_M = (3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
# k_louvain.hip keeps a round in LDS while louvain_round_bytes(m) <= louvain_level0_lds_max()
LDS_ROUND_BYTES_SRC = "inline size_t louvain_round_bytes(int m) { return (size_t)m * (4 * sizeof(double) + 8 * sizeof(int)); }"
LDS_MAX_SRC = "return 160 * 1024 - (int)sizeof(LvShared) - 1024;"
LDS_ROUND_BYTES = 4 * 8 + 8 * 4            # 64 bytes per node
LDS_LAST_M = 2508                          # the largest m in LDS, sizeof(LvShared) = 2272: 64 * 2508 = 160512 <= 160544
SLAB_FIRST_M = 2509                        # 64 * 2509 = 160576 > 160544
SLAB_M = (2400, LDS_LAST_M, SLAB_FIRST_M, 2600)
ROUNDS_MAX = 1024                          # LOUVAIN_MAX_ROUNDS


def _fresh(seeds, rounds):
    return [np.random.default_rng([s, i]).bit_generator.state for s in seeds for i in range(rounds)]


def _case_table():
    t = {}
    for m in CIRCULANT_M:
        t["circulant-%d" % m] = (lambda m=m: circulant(m, CIRCULANT_OFFSETS), lambda: _fresh((0,), 2))
    for m in SLAB_M:
        t["slab-%d" % m] = (lambda m=m: four_groups(m, 13), lambda: _fresh((0,), 3))
    for m in STRIDE_M:
        t["stride-%d" % m] = (lambda m=m: four_groups(m, 17), lambda: _fresh((0, 3), 2))
    t["rounds-1024"] = (lambda: quantised(24, 3, 7), lambda: _fresh((0,), ROUNDS_MAX))
    buffered = lambda: [buffered_state(s, i) for s in (0, 3) for i in range(2)]  # noqa: E731
    t["buffered-planted"] = (lambda: planted([30, 22, 14, 9], 3), buffered)
    t["buffered-circulant-300"] = (lambda: circulant(300, CIRCULANT_OFFSETS), buffered)
    t["zeros-5"] = (lambda: np.zeros((5, 5)), lambda: _fresh((0, 3), 2))
    t["ones-257"] = (lambda: np.ones((257, 257)), lambda: _fresh((0, 3), 2))
    t["isolated"] = (isolated, lambda: _fresh((0, 3), 2))
    t["blocks"] = (blocks, lambda: _fresh((0, 3), 2))
    t["nan-cell"] = (nan_cell, lambda: _fresh((0, 3), 2))
    t["m3"] = (lambda: planted([1, 1, 1], 5), lambda: _fresh((0, 3), 2))
    t["m3-pair"] = (lambda: np.array([[0.0, 5.0, 0.125], [5.0, 0.0, 0.25], [0.125, 0.25, 0.5]]), lambda: _fresh((0, 3), 2))
    return t


LEVEL0_CASES = _case_table()
_level0_cache = {}


def level0_case(name):
    """(A, states, [Level0 per state]) of a named case."""
    if name not in _level0_cache:
        graph, states = LEVEL0_CASES[name]
        A, sts = graph(), states()
        A.setflags(write=False)
        _level0_cache[name] = (A, sts, [trace_level0(A, s) for s in sts])
    return _level0_cache[name]


# ---------------------------------------------------------------- aggregation and score from the definition
def _sorted_by_group(part, k):
    part = np.asarray(part, dtype=np.int64)
    perm = np.argsort(part, kind="stable")
    sizes = np.bincount(part, minlength=k)
    off = np.concatenate(([0], np.cumsum(sizes)))
    return perm, sizes, off


def _int_block_sums(A, part, k):
    """sum of A over (members of a) x (members of b) and the self-loop sums, in integers (7 m^2 stays far below
    2^63, so int64 adds are the exact integers)."""
    Ai = np.asarray(A).astype(np.int64)
    assert np.array_equal(Ai, A)
    perm, sizes, off = _sorted_by_group(part, k)
    Ap = Ai[np.ix_(perm, perm)]
    full = np.flatnonzero(sizes > 0)                 # (reduceat cannot express an empty group)
    B = np.zeros((k, k), dtype=np.int64)
    B[np.ix_(full, full)] = np.add.reduceat(np.add.reduceat(Ap, off[full], axis=0), off[full], axis=1)
    loops = np.zeros(k, dtype=np.int64)
    loops[full] = np.add.reduceat(np.diag(Ap), off[full])
    return B, loops


def induced_exact(A, part, k):
    """The community graph of an integer-valued A, exact: B[a][b] = sum over i in a, j in b of A[i][j] in integers; the
    diagonal is (B[a][a] + the members' self loops) / 2, an integer or a half.  Every value is far below 2^53, so the
    fp64 result has no rounding at all."""
    B, loops = _int_block_sums(A, part, k)
    out = B.astype(np.float64)
    for a in range(k):
        out[a, a] = (int(B[a, a]) + int(loops[a])) / 2          # Python int / int: correctly rounded, here exact
    return out


def induced_fsum(A, part, k):
    """The same from math.fsum per entry (every entry is the correctly rounded sum; the halved diagonal sums the block and
    the self loops in ONE fsum)."""
    import math
    A = np.asarray(A, dtype=np.float64)
    perm, sizes, off = _sorted_by_group(part, k)
    Ap = A[np.ix_(perm, perm)]
    dg = np.diag(Ap)
    out = np.zeros((k, k))
    one = np.flatnonzero(sizes == 1)
    out[np.ix_(one, one)] = Ap[np.ix_(off[one], off[one])]      # 1 x 1 blocks are their own sum
    big = np.flatnonzero(sizes > 1)
    for a in range(k):
        if sizes[a] == 0:
            continue
        for b in (np.flatnonzero(sizes > 0) if sizes[a] > 1 else big):
            out[a, b] = math.fsum(Ap[off[a]:off[a + 1], off[b]:off[b + 1]].ravel().tolist())
    for a in range(k):
        blk = Ap[off[a]:off[a + 1], off[a]:off[a + 1]].ravel().tolist()
        out[a, a] = math.fsum(blk + dg[off[a]:off[a + 1]].tolist()) / 2.0
    return out


def induced_group_sizes(part, k):
    return np.bincount(np.asarray(part, dtype=np.int64), minlength=k)


def modularity_exact(part, A):
    """community.modularity of an integer-valued A as a Fraction: sum over the communities present of
    in_c / links - (deg_c / (2 links))^2, links = (sum A + trace A) / 2, in_c = (sum of A over c x c + c's self loops) / 2,
    deg_c = the members' row sums plus their self loops."""
    from fractions import Fraction
    labels, inv = np.unique(np.asarray(part), return_inverse=True)
    k = len(labels)
    B, loops = _int_block_sums(A, inv, k)
    links = Fraction(int(B.sum()) + int(loops.sum()), 2)
    if links == 0:
        raise ValueError("A graph without link has an undefined modularity")
    q = Fraction(0)
    for c in range(k):
        inc = Fraction(int(B[c, c]) + int(loops[c]), 2)
        deg = int(B[c].sum()) + int(loops[c])
        q += inc / links - (Fraction(deg) / (2 * links)) ** 2
    return q


def modularity_fsum(part, A):
    """The same in longdouble (64-bit mantissa) on the fp64 cells of A; np.longdouble out."""
    L = np.longdouble
    labels, inv = np.unique(np.asarray(part), return_inverse=True)
    k = len(labels)
    perm, sizes, off = _sorted_by_group(inv, k)
    Ap = np.asarray(A, dtype=np.float64)[np.ix_(perm, perm)].astype(L)
    dg = np.diag(Ap).copy()
    links = (Ap.sum() + dg.sum()) / L(2)
    if links == 0:
        raise ValueError("A graph without link has an undefined modularity")
    deg = Ap.sum(axis=1) + dg
    q = L(0)
    for c in range(k):
        s = slice(off[c], off[c + 1])
        inc = (Ap[s, s].sum() + dg[s].sum()) / L(2)
        d = deg[s].sum() / (L(2) * links)
        q += inc / links - d * d
    return q


# ---------------------------------------------------------------- aggregation cases
AGG_M = (1, 2, 255, 256, 257, 1000)
AGG_K = (1, 2, 255, 256, 257)
EPS = 2.0 ** -53


def agg_ks(m):
    return sorted({k for k in AGG_K + (m,) if k <= m})


def agg_graph(m, exact):
    """Symmetric weights: integers 0..7 (every sum exact) or rng.random (every sum rounds).  A[0][0] > 0, so the
    graph has a link at every m."""
    rng = np.random.default_rng([41, m, int(exact)])
    if exact:
        a = rng.integers(0, 8, (m, m)).astype(np.float64)
        a = np.triu(a) + np.triu(a, 1).T
        a[0, 0] = 3.0
    else:
        a = rng.random((m, m))
        a = np.triu(a) + np.triu(a, 1).T
        a[0, 0] += 0.25
    assert np.array_equal(a, a.T)
    return a


def agg_partitions(m, k):
    """name -> labels in [0, k): all in one, i % k, contiguous blocks, two random ones (communities may stay empty),
    identity (k == m), and i % k with the middle community emptied into community 0 (k >= 3).  At least five."""
    i = np.arange(m)
    rng = np.random.default_rng([43, m, k])
    parts = {"one": np.zeros(m, np.int64), "mod": i % k, "blocks": i * k // m, "random": rng.integers(0, k, m),
             "random2": rng.integers(0, k, m)}
    if k == m:
        parts["identity"] = i.copy()
    if k >= 3:
        p = i % k
        p[p == k // 2] = 0
        parts["hole"] = p
    return parts
