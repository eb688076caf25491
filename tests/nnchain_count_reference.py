"""An independent count of what SciPy's nn_chain does for 'average' linkage: a plain NumPy restatement of
scipy/cluster/_hierarchy.pyx nn_chain that returns, besides the raw merges, how many CHAIN STEPS the loop took and how many
columns those steps visited.  The nn-chain kernels report the same two quantities (hicmi_nnchain_stats: row scans, scan
columns, chain steps answered by the neighbour cache); tests/test_gpu_timing.py compares them with this count, and
tests/test_timing_cpu.py pins this file against SciPy and against the oracle's C port.

A chain step is one pass of SciPy's inner loop: the row of the chain's top element is scanned over the live clusters - the
one pass that confirms a reciprocal pair included.  At merge `step` (0-based) n - step clusters are alive, and that is what a
step visits (the kernels count total_steps + 1 - step, the row's own column included).

Semantics that decide the counts, as in SciPy:
  * an empty chain starts at the first live index;
  * with a chain longer than one the previous element's distance is the incumbent: only a STRICTLY smaller distance
    replaces it, and among equal minima the first (lowest index) wins;
  * the smaller index dies, the larger keeps the Lance-Williams average (nx * d(i, x) + ny * d(i, y)) / (nx + ny) - two
    products, a sum, a quotient, each rounded;
  * only the strict upper triangle of the distance matrix is read (squareform of a matrix takes d[i, j], i < j).
"""
import numpy as np


def random_contacts(n, seed):
    """The symmetric random map of the nn-chain parity tests (tests/test_gpu_parity.py)."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, n)) + 0.01
    return c + c.T


def all_ties_contacts(n, seed):
    """The integer map of test_upgma_without_neighbour_cache_bit_exact: three distinct values, ties in every row.  (That
    test draws it from the generator that has already produced the random map.)"""
    rng = np.random.default_rng(seed)
    rng.random((n, n))
    t = rng.integers(1, 4, size=(n, n)).astype(np.float64)
    return np.triu(t, 1) + np.triu(t, 1).T + np.eye(n)


def nn_chain_counted(dist):
    """dist: n x n float64, d[i, j] for i < j is used.  Returns (zraw, steps, columns): the (n - 1) x 4 merges in merge
    order (x, y, height, size) with x < y the slots that merged, the number of chain steps, and the sum over those steps of
    the live clusters at that moment."""
    dist = np.asarray(dist, dtype=np.float64)
    n = dist.shape[0]
    zraw = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
    if n < 2:
        return zraw, 0, 0
    up = np.triu(dist, 1)
    d = up + up.T                                   # every pair's one distance, both ways round
    np.fill_diagonal(d, np.inf)                     # a row never meets itself; dead slots are set to +inf below
    size = np.ones(n, dtype=np.int64)
    chain = []
    steps = columns = 0
    for step in range(n - 1):
        live = n - step
        if not chain:
            chain.append(int(np.flatnonzero(size > 0)[0]))
        while True:
            x = chain[-1]
            steps += 1
            columns += live
            row = d[x]
            i = int(np.argmin(row))                 # first minimum over the live columns (the others hold +inf)
            if len(chain) > 1:
                y, cur = chain[-2], row[chain[-2]]
                if row[i] < cur:
                    y, cur = i, row[i]
            else:
                y, cur = i, row[i]
            if len(chain) > 1 and y == chain[-2]:
                break
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        zraw[step] = (x, y, cur, nx + ny)
        size[x], size[y] = 0, nx + ny
        new = (float(nx) * d[x] + float(ny) * d[y]) / float(nx + ny)
        alive = size > 0
        alive[y] = False
        d[y, alive] = new[alive]
        d[alive, y] = new[alive]
        d[x, :] = np.inf
        d[:, x] = np.inf
    return zraw, steps, columns
