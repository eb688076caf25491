"""Cases for Part 2's insertion phase and scan loops, and a thin driver over hic_oracle.Part2Oracle.

A case is a symmetric fp64 matrix, the scaffolds' bin counts over consecutive bins (scaffold i = device scaffold id i),
a starting arrangement and the scaffolds to insert, in order.  The driver calls Part2Oracle.check_all_scores and
Part2Oracle.scan_ordering as they are and reads the literal costs of every step from Part2Oracle.costs; it states
neither the objective nor the decision rule again.  Every case is built to reach one branch of the device path
(k_part2_insert.hip); tests/test_insertion_cpu.py proves from the oracle's costs alone that it does.
"""
import functools
from collections import namedtuple

import numpy as np

import hic_oracle as orc

NEAR_TOP = 1e-9                   # api.hip's kNearTop: the relative band of the short lists
PROBE_LENS = (9, 7, 6, 5, 4, 3, 3, 2, 2, 1, 1, 1)

Case = namedtuple("Case", "name mat lens ids0 rev0 new_ids")
Step = namedtuple("Step", "ids_before rev_before new_id costs gap rev best decided ids rev_after")
Insertion = namedtuple("Insertion", "steps ids rev best")
Scan = namedtuple("Scan", "ids0 rev0 best0 total ids rev best rounds")


class _Bin:
    def __init__(self, ID):
        self.ID = ID


# ---------------------------------------------------------------------------------------------- matrices
def smooth_map(n, seed=5):
    """gamma(2, 1) / (1 + |i - j|), made symmetric: contacts that fall off with distance, no two equal."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    c = rng.gamma(2.0, 1.0, size=(n, n)) / (1.0 + np.abs(i[:, None] - i[None, :]))
    return np.ascontiguousarray(0.5 * (c + c.T))


def scaffold_of_bin(lens):
    return np.repeat(np.arange(len(lens)), lens)


def block_diagonal(mat, lens):
    """``mat`` with every contact between two different scaffolds set to 0."""
    s = scaffold_of_bin(lens)
    return np.ascontiguousarray(np.where(s[:, None] == s[None, :], mat, 0.0))


def isolate(mat, lens, sid):
    """``mat`` with every contact between scaffold ``sid`` and another scaffold set to 0."""
    s = scaffold_of_bin(lens)
    mine = s == sid
    out = mat.copy()
    out[np.ix_(mine, ~mine)] = 0.0
    out[np.ix_(~mine, mine)] = 0.0
    return out


def quantise(mat):
    c = np.floor(3.0 * mat)
    return np.ascontiguousarray(0.5 * (c + c.T))


# ---------------------------------------------------------------------------------------------- insertion cases
def _probe_case(name, mat, lens=PROBE_LENS, s0=4):
    return Case(name, mat, tuple(lens), tuple(range(s0)), (0,) * s0, tuple(range(s0, len(lens))))


def case_generic():
    return _probe_case("generic", smooth_map(sum(PROBE_LENS)))


def case_isolated(bins):
    """The probe map with one scaffold of ``bins`` (2 or 1) bins cut off from every other scaffold."""
    sid = {2: 7, 1: 9}[bins]
    assert PROBE_LENS[sid] == bins
    return _probe_case("isolated-%d-bin" % bins, isolate(smooth_map(sum(PROBE_LENS)), PROBE_LENS, sid))


def case_block_diagonal():
    return _probe_case("block-diagonal", block_diagonal(smooth_map(sum(PROBE_LENS)), PROBE_LENS))


BLOCK_SMALL_LENS = (4, 3, 3, 2, 1, 1, 1, 1, 1)


def case_block_diagonal_small():
    """One-bin scaffolds inserted at S = 4 ... 7 (lists of 10 ... 16, halved by the twin rule) and one at S = 8 (18)."""
    lens = BLOCK_SMALL_LENS
    return _probe_case("block-diagonal-small", block_diagonal(smooth_map(sum(lens)), lens), lens)


def case_no_contacts():
    return _probe_case("no-contacts", np.eye(sum(PROBE_LENS)))


def case_constant():
    return _probe_case("constant", np.ones((sum(PROBE_LENS),) * 2))


def case_quantised():
    return _probe_case("quantised", quantise(smooth_map(sum(PROBE_LENS))))


def case_256_scaffolds():
    """270 scaffolds of 1 - 2 bins: 250 arranged (shuffled, some flipped), then 12 more, so S runs 250 ... 261."""
    rng = np.random.default_rng(256)
    lens = tuple(int(v) for v in rng.integers(1, 3, size=270))
    ids0 = rng.permutation(250)
    rev0 = rng.integers(0, 2, size=250)
    return Case("256-scaffolds", smooth_map(sum(lens), seed=6), lens, tuple(int(v) for v in ids0),
                tuple(int(v) for v in rev0), tuple(range(250, 262)))


BINS_8192_LENS = (4096, 4090, 5, 1, 1, 2)


@functools.lru_cache(maxsize=1)
def case_8192_bins():
    """Arrangements of 8191, 8192 and 8193 bins at the three steps: either side of both 8192-value LDS staging limits."""
    n = sum(BINS_8192_LENS)
    m = np.random.default_rng(8192).random((n, n))
    m += m.T.copy()
    return Case("8192-bins", m, BINS_8192_LENS, (0, 1, 2), (0, 1, 0), (3, 4, 5))


SMALL_CASES = {
    "generic": case_generic,
    "isolated-2-bin": lambda: case_isolated(2),
    "isolated-1-bin": lambda: case_isolated(1),
    "block-diagonal": case_block_diagonal,
    "block-diagonal-small": case_block_diagonal_small,
    "no-contacts": case_no_contacts,
    "constant": case_constant,
    "quantised": case_quantised,
    "256-scaffolds": case_256_scaffolds,
}
ALL_CASES = dict(SMALL_CASES, **{"8192-bins": case_8192_bins})


def first_steps(case, count):
    """``case`` cut down to its first ``count`` insertions."""
    return case._replace(name="%s-first-%d" % (case.name, count), new_ids=case.new_ids[:count])


# ---------------------------------------------------------------------------------------------- the oracle driver
def _oracle(case):
    """(Part2Oracle over the whole matrix, its Scaffold objects by device id).  _use_group is not called: the objective
    then reads the case's matrix itself (no second copy of the 8192-bin one), with bin ID = matrix index."""
    n = case.mat.shape[0]
    o = orc.Part2Oracle(case.mat, [_Bin(i) for i in range(n)])
    starts = np.concatenate([[0], np.cumsum(case.lens)]).astype(int)
    scaffs = [orc.Scaffold(i, list(range(starts[i], starts[i + 1])), "+") for i in range(len(case.lens))]
    return o, scaffs


def _arranged(scaffs, ids, rev):
    out = []
    for i, r in zip(ids, rev):
        if (scaffs[i].orientation == "-") != bool(r):
            scaffs[i].flipOrientation()
        out.append(scaffs[i])
    return out


def _describe(ordered):
    return (np.array([s.name for s in ordered], np.int32), np.array([s.orientation == "-" for s in ordered], np.uint8))


def run_insertion(case, enter_flipped=False):
    """check_all_scores for every scaffold of ``case.new_ids``.  Per step: the arrangement before it, the 2 (S + 1)
    literal costs in enumeration order, the chosen gap and orientation (reversed flag), ``best``, whether any cost was
    above 0 (``decided``), and the arrangement after it.  ``enter_flipped``: every new scaffold enters as '-'."""
    o, scaffs = _oracle(case)
    ordered = _arranged(scaffs, case.ids0, case.rev0)
    steps = []
    for nid in case.new_ids:
        new = scaffs[nid]
        if enter_flipped:
            new.flipOrientation()
        before = _describe(ordered)
        n0 = len(o.costs)
        ordered, best = o.check_all_scores(ordered, new)
        costs = np.array(o.costs[n0:], np.float64)
        assert len(costs) == 2 * (len(before[0]) + 1)
        after = _describe(ordered)
        gap = [s.name for s in ordered].index(nid)
        steps.append(Step(before[0], before[1], nid, costs, gap, int(after[1][gap]), best,
                          bool(np.any(costs > 0.0)), after[0], after[1]))
    return Insertion(steps, steps[-1].ids, steps[-1].rev_after, steps[-1].best)


@functools.lru_cache(maxsize=None)
def reference(name):
    """run_insertion of a named case, computed once per process and shared (treat it as read-only)."""
    return run_insertion(ALL_CASES[name]())


def by_gap_rev(step, enter_flipped=False):
    """A step's literal costs in hicmi_p2_score_insertions' layout [2 gap + reversed flag].  The enumeration tests gap g in
    the orientation the scaffold left gap g - 1 with, then flipped: costs[2 g] is orientation (g & 1) ^ entered."""
    out = np.empty_like(step.costs)
    for g in range(len(step.costs) // 2):
        o = (g & 1) ^ int(bool(enter_flipped))
        out[2 * g + o] = step.costs[2 * g]
        out[2 * g + (o ^ 1)] = step.costs[2 * g + 1]
    return out


def near_top_count(costs, floor=0.0):
    """How many finite costs lie within the short lists' relative band of max(best cost, floor)."""
    ok = np.isfinite(costs)
    if not ok.any():
        return 0
    top = max(float(costs[ok].max()), floor)
    return int(np.count_nonzero(ok & (costs >= top - abs(top) * NEAR_TOP)))


# ---------------------------------------------------------------------------------------------- scan cases
ScanCase = namedtuple("ScanCase", "name mat lens k")


def _scan_probe(k, S=len(PROBE_LENS)):
    lens = PROBE_LENS[:S]
    return ScanCase("probe-S%d-k%d" % (S, k), smooth_map(sum(PROBE_LENS))[:sum(lens), :sum(lens)].copy(), lens, k)


SCAN_CASES = {
    "probe-k2": lambda: _scan_probe(2),
    "probe-k3": lambda: _scan_probe(3),
    "probe-k5": lambda: _scan_probe(5),
    "S3-k3": lambda: _scan_probe(3, 3),
    "S4-k3": lambda: _scan_probe(3, 4),
    "block-diagonal-k3": lambda: ScanCase("block-diagonal-k3", case_block_diagonal().mat, PROBE_LENS, 3),
    "constant-k3": lambda: ScanCase("constant-k3", case_constant().mat, PROBE_LENS, 3),
}


def scan_start(S):
    """The shuffled start of every scan case: a default_rng(1) permutation with random flips."""
    rng = np.random.default_rng(1)
    return rng.permutation(S).astype(np.int32), rng.integers(0, 2, size=S).astype(np.uint8)


def run_scan(case):
    """scan_ordering from scan_start with best0 = the literal cost of the start.  ``rounds`` is the number of
    evaluations divided by the evaluations of one round."""
    o, scaffs = _oracle(Case(case.name, case.mat, case.lens, (), (), ()))
    S, k = len(case.lens), case.k
    ids0, rev0 = scan_start(S)
    ordered = _arranged(scaffs, ids0, rev0)
    row = o._global(ordered)
    total = o.total(row)
    best0 = o.cost(row, total)
    n0 = len(o.costs)
    ordered, best = o.scan_ordering(ordered, {s.name: s for s in scaffs}, best0, k)
    per_round = (S - k + 1) * len(orc.remove_reverse_duplicates(orc.swap_permutations(list(range(k))))) \
        * len(orc.plus_minus_perms(k))
    evals = len(o.costs) - n0
    assert evals % per_round == 0
    ids, rev = _describe(ordered)
    return Scan(ids0, rev0, best0, total, ids, rev, best, evals // per_round)


@functools.lru_cache(maxsize=None)
def scan_reference(name):
    return run_scan(SCAN_CASES[name]())
