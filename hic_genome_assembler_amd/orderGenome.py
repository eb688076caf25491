"""Part 2 (order + orient scaffolds inside each chromosome) on MI355X: drop-in for the reference
module of the same name (/root/reference/HIC_ASSEMBLER/orderGenome.py, OG below).

Same ``runPipeline`` signature, same input/output files and the same search - brute force over the
largest scaffolds, greedy insertion of the rest, sliding-window re-permutation to a fixed point -
with the reference's enumeration order and first-strict-maximum tie-breaking.  What changes is where
candidates live and how they are scored:

* a chromosome's contacts are selected ONCE into a device sub-matrix; each scaffold is a contiguous
  range of it (the layout) and an order/orientation is a list of (scaffold, reversed) pairs (the
  arrangement) - the reference instead rebuilds a gathered matrix and an index dictionary for every
  step (giveNewAdjMat, OG:296-308) and a Python index list per candidate;
* the candidates of a step are enumerated by the kernels themselves (k_part2_search.hip):
  2(S+1) insertions per launch, k!/2 * 2^k window candidates per launch with the incremental form
  of the objective;
* the few candidates that can win a step are re-scored in the reference's exact operation order
  (k_p2_diag_sums), because `cost > bestCost` is decided at the last bit (see first_strict_max).
"""
from __future__ import annotations

import math
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib
from . import plotContactMaps as plotModule
from .hostio import Bin, initiateLoci, paused_gc, read_contact_matrix, read_contact_matrix_cached  # noqa: F401

SCORE_HOOK = None      # tests: called with the fast scores of every step, in enumeration order
_PROFILE = bool(os.environ.get("HICMI_PART2_PROFILE"))   # per-chromosome wall clock on stderr
WORKERS = int(os.environ.get("HICMI_PART2_WORKERS", "8"))
LOCKSTEP = os.environ.get("HICMI_PART2_LOCKSTEP", "1") != "0"   # all chromosomes' insertion loops in one queue of launches   # chromosomes ordered concurrently (1 = sequential)
START_THREADS = int(os.environ.get("HICMI_PART2_START_THREADS", "0"))   # A/B: the start phase on this many threads (0: the calling thread)
START_ALL = os.environ.get("HICMI_PART2_START_ALL", "1") != "0"   # A/B: every chromosome's start phase in ONE native call (0: one after the other)
SCAN_ARRANGED = os.environ.get("HICMI_PART2_SCAN_ARRANGED", "1") != "0"   # A/B: the scan entered with the insertion's ids / rev (0: through Scaffold objects)
NEAR_TOP = 1e-9        # relative band around a step's best fast score that is re-scored literally


# ------------------------------------------------------------------------------------------------
class GenomeMatrix:
    """Raw contacts of the grouped bins, resident on the GPU (OG:690)."""

    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx
        self.chrom = None              # ChromosomeLayout currently selected on the device
        self._bin_index = None
        self._bin_index_src = None

    def __len__(self):
        return self.ctx.n

    def bin_index(self, binList):
        if self._bin_index is None or self._bin_index_src is not binList:
            self._bin_index = {b.ID: i for i, b in enumerate(binList)}
            self._bin_index_src = binList
        return self._bin_index

    def lanes(self, count):
        """This matrix and ``count`` - 1 more on worker contexts (own HIP stream, own scratch) that read the same
        device-resident contacts and share the bin index: one per job in flight."""
        out = [self] + [GenomeMatrix(c) for c in self.ctx.workers(count - 1)]
        for m in out[1:]:
            m._bin_index, m._bin_index_src = self._bin_index, self._bin_index_src
        return out

    def select(self, layout):
        """Make ``layout`` the chromosome selected on the device again (a context that served several layouts in turn)."""
        if self.chrom is not layout:
            layout.issue()
            self.chrom = layout


class ChromosomeLayout:
    """All scaffolds of one chromosome selected on the device: scaffold s <-> a contiguous range of
    the selection holding its bins in ascending-ID ('+') order."""

    def __init__(self, matrix: GenomeMatrix, scaffolds, binList, issue=True):
        """``issue=False``: only the host side - the selection and the ranges are handed to the device by the caller
        (hicmi_p2_start_all takes ``sel``, ``start`` and ``length`` of all chromosomes at once)."""
        self.ctx = matrix.ctx
        where = matrix.bin_index(binList)
        self.sid, self.start, self.length, self.names = {}, [], [], []
        sel, pos = [], 0
        for s in scaffolds:
            bins = sorted(s.binList)
            self.sid[s.name] = len(self.start)
            self.names.append(s.name)
            self.start.append(pos)
            self.length.append(len(bins))
            sel.extend(map(where.__getitem__, bins))
            pos += len(bins)
        self.n = pos
        self.sel = sel
        self._pos_cache = {}
        self._tables_k = None
        if issue:
            self.issue()

    def issue(self):
        self.ctx.p2_select(self.sel)
        self.ctx.p2_layout(self.start, self.length)
        self._tables_k = None

    def whole_total(self):
        """The total of the whole selection: every scaffold in layout order, '+' (the one footing on which different
        arrangements of the chromosome compare)."""
        if self.n < 2:
            return 0.0
        S = len(self.start)
        self.ctx.p2_set_arrangement(np.arange(S, dtype=np.int32), np.zeros(S, np.uint8))
        return self.ctx.p2_arrangement_total()

    def covers(self, scaffs):
        return all(s.name in self.sid for s in scaffs)

    def describe(self, scaffs):
        """(ids, rev) of an arrangement; rev = 1 for '-'."""
        ids = np.fromiter((self.sid[s.name] for s in scaffs), dtype=np.int32, count=len(scaffs))
        rev = np.fromiter((1 if s.orientation == "-" else 0 for s in scaffs), dtype=np.uint8, count=len(scaffs))
        return ids, rev

    def positions(self, sid, rev):
        """Selection indices of one scaffold laid down forward / reversed (cached)."""
        key = (sid, bool(rev))
        hit = self._pos_cache.get(key)
        if hit is None:
            a = np.arange(self.start[sid], self.start[sid] + self.length[sid], dtype=np.int32)
            hit = self._pos_cache[key] = np.ascontiguousarray(a[::-1]) if rev else a
        return hit

    def node_row(self, ids, rev):
        return np.concatenate([self.positions(int(i), int(r)) for i, r in zip(ids, rev)]) if len(ids) else \
            np.zeros(0, np.int32)

    def tables(self, k):
        if self._tables_k != k:
            orders, orients = _enumeration(k)
            self.ctx.p2_window_tables(np.asarray(orders, dtype=np.int8),
                                      np.asarray([[1 if sg == "-" else 0 for sg in r] for r in orients], dtype=np.uint8))
            self._tables_k = k
        return _enumeration(k)


class SubMatrix:
    """What giveNewAdjMat returns here: the scaffolds of ``scaffList`` in their order and
    orientation AT CREATION (that order fixes the rounding of ``total``, OG:343/448/506), plus a
    cache of literal scores evaluated under that total."""

    def __init__(self, layout: ChromosomeLayout, scaffList):
        self.layout = layout
        self.ctx = layout.ctx
        self.ids, self.rev = layout.describe(scaffList)
        self.n = int(sum(layout.length[i] for i in self.ids))
        self._total = None
        self.exact = {}                # node-row bytes -> literal score under this total

    def __len__(self):
        return self.n

    def total(self) -> float:
        """Sum of everything above the diagonal with the reference's rounding (OG:343, 448, 506)."""
        if self._total is None:
            if self.n < 2:
                self._total = 0.0
            else:
                self.ctx.p2_set_arrangement(self.ids, self.rev)
                self._total = self.ctx.p2_arrangement_total()
        return self._total

    def first_strict_max(self, fast, floor, row_of):
        """The reference's ``if cost > bestCost`` scan over a step's candidates in enumeration order
        (OG:349,359,464,535), starting from ``bestCost = floor``: returns (index, cost) of the winner
        or (-1, floor).

        ``fast`` are the closed-form fp64 scores of all candidates; ``row_of(c)`` gives candidate c's
        bin order as selection indices.  The reference's comparisons are decided at the last bit -
        the same arrangement scored under two differently rounded totals (OG:506 vs OG:343) differs
        by an ulp, and that decides whether a pass "improves" - so every candidate within 1e-9 of
        the step's best is re-scored in the reference's exact operation order
        (hicmi_p2_score_exact) and the decision is taken on those values.  Identical bin orders
        (flipping a one-bin scaffold) share one literal evaluation and tie exactly, as they do in
        the reference."""
        fast = np.asarray(fast, dtype=np.float64)
        if SCORE_HOOK is not None:
            SCORE_HOOK(fast)
        ok = np.isfinite(fast)
        if not ok.any():
            return -1, floor
        top = max(float(fast[ok].max()), float(floor))
        near = np.flatnonzero(ok & (fast >= top - abs(top) * NEAR_TOP))
        if len(near) == 0:
            return -1, floor
        rows = [np.ascontiguousarray(row_of(int(c)), dtype=np.int32) for c in near]
        keys = [r.tobytes() for r in rows]
        todo = {}
        for r, key in zip(rows, keys):
            if key not in self.exact and key not in todo:
                todo[key] = r
        if todo:
            if len(rows[0]) < 2:
                vals = np.zeros(len(todo))                       # range(1, 1) is empty: cost 0.0
            else:
                vals = self.ctx.p2_score_exact(np.stack(list(todo.values())), self.total())
            for key, v in zip(todo, vals):
                self.exact[key] = float(v)
        pick, best = -1, floor
        for c, key in zip(near, keys):
            v = self.exact[key]
            if v > best:
                pick, best = int(c), v
        return pick, best


def buildAdjacencyMatrix(matrixFile, binList, binID_dict=False, device=0, ctx=None):
    """OG:65-93."""
    cache = os.environ.get("HICMI_MATRIX_CACHE")           # "1": beside the text file; or a directory (hostio.py)
    host = read_contact_matrix_cached(matrixFile, binList, cache) if cache else read_contact_matrix(matrixFile, binList)
    ctx = ctx or _lib.Context(device)
    ctx.set_contacts(host)
    print("Rows in adjacency matrix " + str(len(binList)))
    return GenomeMatrix(ctx)


def readGroupingsToValidBins(chromosomeGroupFile):
    """OG:200-214."""
    ids = {}
    with open(chromosomeGroupFile) as fh:
        for line in fh:
            line = line.strip("\r").strip("\n")
            if line[0] != "#":
                ids[int(line.split("\t")[0])] = ''
    return ids


def readChromsFromFile(inFile):
    """OG:216-237."""
    chroms, cur = [], []
    with open(inFile) as fh:
        fh.readline()
        text = fh.read()
    if "\r" in text:                                   # rare: keep the reference's exact stripping (OG:222)
        lines = [ln.strip("\r").strip("\n") for ln in text.splitlines(keepends=True)]
    else:
        lines = text.split("\n")
        if lines and lines[-1] == "":                   # the file's final newline
            lines.pop()
    add = cur.append
    for line in lines:
        if line[0] != "#":
            cols = line.split("\t", 2)
            add([int(cols[0]), cols[1]])
        else:
            chroms.append(cur)
            cur = []
            add = cur.append
    chroms.append(cur)
    print("Chromosomes found " + str(len(chroms)))
    print("Nodes found " + str(sum(len(c) for c in chroms)))
    return chroms


class Scaffold:
    """OG:239-254: name, bins in 5'->3' order of the current orientation, orientation sign."""

    def __init__(self, name, binList, orientation):
        self.name = name
        self.binList = binList
        self.orientation = orientation

    def flipOrientation(self):
        self.orientation = "-" if self.orientation == "+" else "+"
        self.binList = self.binList[::-1]

    def copy(self):
        out = Scaffold(self.name, list(self.binList), self.orientation)
        out.nodeCount = getattr(self, "nodeCount", len(self.binList))
        return out


def initiateBinsAndScaffolds(nodeList, quiet=False):
    """OG:256-280: scaffolds in order of first appearance, bins ascending, then a stable sort by
    bin count, largest first.  ``quiet``: the caller prints the "Scaffolds to order" line itself."""
    bins_of = {}
    for bin_id, name in nodeList:
        b = bins_of.get(name)
        if b is None:
            bins_of[name] = [bin_id]
        else:
            b.append(bin_id)
    scaffDict = {name: Scaffold(name, sorted(b), "+") for name, b in bins_of.items()}      # (order of first appearance)
    if not quiet:
        print("Scaffolds to order for this chromosome " + str(len(scaffDict)))
    for s in scaffDict.values():
        s.nodeCount = len(s.binList)
    scaffList = sorted(scaffDict.values(), key=lambda s: len(s.binList), reverse=True)
    return scaffList, scaffDict


def pullScaffolds(puller, pullee, scaffsToPull):
    """OG:282-294."""
    for _ in range(scaffsToPull):
        if len(pullee) == 0:
            break
        puller.append(pullee.pop(0))
    return puller, pullee


def giveNewAdjMat(matrix: GenomeMatrix, scaffList, binList):
    """OG:296-308.  The device already holds the chromosome's sub-matrix (selected once by
    orderChromosome); this records ``scaffList``'s order/orientation - which fixes how ``total`` is
    rounded - and returns it with {binID: index in that order}.  Called outside orderChromosome it
    selects just these scaffolds."""
    if matrix.chrom is None or not matrix.chrom.covers(scaffList):
        matrix.chrom = ChromosomeLayout(matrix, scaffList, binList)
    return SubMatrix(matrix.chrom, scaffList), _OrderDict(scaffList)


class _OrderDict(dict):
    """{binID: index in the sub-matrix} of giveNewAdjMat (OG:302), filled on first use: the device
    path never needs it, only callers of the reference's function-level API do."""

    def __init__(self, scaffList):
        super().__init__()
        self._nodes = [n for s in scaffList for n in s.binList]
        self._filled = False

    def _fill(self):
        if not self._filled:
            self._filled = True
            self.update((b, i) for i, b in enumerate(self._nodes))

    def __getitem__(self, k):
        self._fill()
        return dict.__getitem__(self, k)

    def __len__(self):
        self._fill()
        return dict.__len__(self)

    def __iter__(self):
        self._fill()
        return dict.__iter__(self)

    def __contains__(self, k):
        self._fill()
        return dict.__contains__(self, k)


def reorderScaffList(orderList, orientationList, scaffDict):
    """OG:310-321."""
    scaffs, nodes = [], []
    for name, orient in zip(orderList, orientationList):
        s = scaffDict[name]
        if s.orientation != orient:
            s.flipOrientation()
        scaffs.append(s)
        nodes += s.binList
    return scaffs, nodes


def costFunction(matrix, total):
    """OG:323-330 for an explicit (already permuted) host matrix: uploaded and scored on the GPU in
    the reference's operation order.  Kept for callers of the reference's function-level API."""
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64))
    if len(m) < 2:
        return 0.0
    with _lib.Context(0) as ctx:
        ctx.set_contacts(m)
        ident = np.arange(len(m), dtype=np.int32)
        ctx.p2_select(ident)
        return float(ctx.p2_score_exact(ident[None, :], float(total))[0])


costFunction_numba = costFunction      # OG:184-191


def calcPossiblePerms(N):
    """OG:374-379."""
    return math.factorial(N) * (2 ** N) / 2


# ---- enumeration order (defines tie-breaking) --------------------------------------
def permutations(elementList, paths, k=0):
    """OG:381-394: every order of ``elementList``, in the order produced by swapping position k with
    each later position and recursing."""
    if k == len(elementList):
        paths.append(list(elementList))
        return paths
    for i in range(k, len(elementList)):
        elementList[k], elementList[i] = elementList[i], elementList[k]
        permutations(elementList, paths, k + 1)
        elementList[k], elementList[i] = elementList[i], elementList[k]
    return paths


def removeReverseDuplicates(permList):
    """OG:396-411: of each (order, reversed order) pair keep whichever was enumerated first."""
    pending, kept = set(), []
    for p in permList:
        key = tuple(p)
        if key[::-1] in pending:
            pending.discard(key[::-1])
        else:
            pending.add(key)
            kept.append(p)
    return kept


def plusMinusPerms(elementList):
    """OG:413-430: all-plus first, then for i = 0..k-1 the distinct arrangements of i '+' and k-i '-'
    in swap-enumeration order."""
    k = len(elementList)
    seen, out = set(), []
    for cand in [["+"] * k] + [p for i in range(k) for p in permutations(["+"] * i + ["-"] * (k - i), [], 0)]:
        key = tuple(cand)
        if key not in seen:
            seen.add(key)
            out.append(list(cand))
    return out


_ENUM_CACHE = {}


def _enumeration(k):
    """(orders over slots 0..k-1, orientations), cached.  orders[0] is the identity."""
    if k not in _ENUM_CACHE:
        orders = removeReverseDuplicates(permutations(list(range(k)), [], 0))
        orients = plusMinusPerms(list(range(k)))
        _ENUM_CACHE[k] = (orders, orients, {tuple(r): i for i, r in enumerate(orients)})
    return _ENUM_CACHE[k][0], _ENUM_CACHE[k][1]


_TABLE_CACHE = {}


def _table_arrays(k):
    """_enumeration(k) as the arrays the library takes: orders (int8), orientations (uint8, 1 = '-')."""
    if k not in _TABLE_CACHE:
        orders, orients = _enumeration(k)
        _TABLE_CACHE[k] = (np.asarray(orders, dtype=np.int8),
                           np.asarray([[1 if sg == "-" else 0 for sg in r] for r in orients], dtype=np.uint8))
    return _TABLE_CACHE[k]


def _orient_index(k, signs):
    _enumeration(k)
    return _ENUM_CACHE[k][2][tuple(signs)]


def _window_scores(view: SubMatrix, arrangement, first, k, known_fast=None):
    """Fast scores of all k!/2 * 2^k candidates for the window arrangement[first:first+k] (everything
    else fixed), from one hicmi_p2_score_window launch.  Returns (fast, row_of)."""
    layout, ctx = view.layout, view.ctx
    orders, orients = layout.tables(k)
    ids, rev = layout.describe(arrangement)
    total = view.total()
    ctx.p2_set_arrangement(ids, rev)
    delta = ctx.p2_score_window(first, k)
    if k == len(arrangement):
        fast = delta / total                              # nothing outside the window
    else:
        c0 = _orient_index(k, [s.orientation for s in arrangement[first:first + k]])   # orders[0] = identity
        base = ctx.p2_arrangement_score(total) if known_fast is None else known_fast
        fast = base + (delta - delta[c0]) / total
    n_ori = len(orients)
    win = ids[first:first + k]
    ends = []

    def row_of(c):
        if not ends:                                      # built only if a candidate gets short-listed
            ends.append(layout.node_row(ids[:first], rev[:first]))
            ends.append(layout.node_row(ids[first + k:], rev[first + k:]))
        o, r = orders[c // n_ori], orients[c % n_ori]
        mid = [layout.positions(int(win[j]), sg == "-") for j, sg in zip(o, r)]
        return np.concatenate([ends[0]] + mid + [ends[1]])
    return fast, row_of


def _fused(ctx):
    """Use the one-call decision steps of libhicmi (hicmi_p2_decide_*) unless a test wants to see
    every fast score (SCORE_HOOK) or the context is a test double without them."""
    return SCORE_HOOK is None and hasattr(ctx, "p2_decide_window")


# ---- search ---------------------------------------------------------------------------------------
def bruteForceBestScore(sObjList, scaffDict, matrix: SubMatrix, orderDict):
    """OG:432-473: all k!/2 orders x 2^k orientations of the k largest scaffolds in one launch."""
    names = [s.name for s in sObjList]
    k = len(names)
    orders, orients = _enumeration(k)
    total = matrix.total()
    if total == 0:
        print("WARNING/ERROR - Zero contact values found between scaffolds assigned to chromosome group "
              + ",".join(str(e) for e in names))
        return [names[i] for i in orders[0]], list(orients[0]), 0.0
    print("Initial permutations to test " + str(len(orders) * len(orients)) + "...")
    if _fused(matrix.ctx):
        matrix.layout.tables(k)
        matrix.ctx.p2_set_arrangement(*matrix.layout.describe(sObjList))
        best, best_c, _pf = matrix.ctx.p2_decide_window(0, k, total, 0., None)
    else:
        fast, row_of = _window_scores(matrix, sObjList, 0, k)
        best, best_c = matrix.first_strict_max(fast, 0., row_of)      # first strict maximum above 0. (OG:464)
    # the enumeration leaves every scaffold in the last candidate's orientation (OG:459)
    reorderScaffList([names[i] for i in orders[-1]], orients[-1], scaffDict)
    if best < 0:
        raise RuntimeError("no candidate order scored above 0 (the reference fails here too, OG:473 -> OG:576)")
    o, r = orders[best // len(orients)], orients[best % len(orients)]
    return [names[i] for i in o], list(r), best_c


def checkAllScores(adjMat: SubMatrix, orderDict, orderedScaffs, scaffToCheck):
    """OG:332-372: try the scaffold at every gap, both orientations.  The scaffold is flipped once
    per gap and stays flipped, so the orientation tried first alternates with the gap index."""
    layout, ctx = adjMat.layout, adjMat.ctx
    gaps = len(orderedScaffs) + 1
    flip = {"+": "-", "-": "+"}
    new_id = layout.sid[scaffToCheck.name]
    ids, rev = layout.describe(orderedScaffs)
    if _fused(ctx) and len(ids) > 0:
        gap, r, bestCost = ctx.p2_decide_insertion(ids, rev, new_id, scaffToCheck.orientation == "-")
        bestGap, bestOrient = (gap, "-" if r else "+") if gap >= 0 else (0, "+")
        if gaps % 2 == 1:                               # one flip per gap (OG:356)
            scaffToCheck.flipOrientation()
        if scaffToCheck.orientation != bestOrient:
            scaffToCheck.flipOrientation()
        orderedScaffs.insert(bestGap, scaffToCheck)
        return orderedScaffs, bestCost
    total = adjMat.total()
    tags, o = [], scaffToCheck.orientation
    for i in range(gaps):
        tags += [(i, o), (i, flip[o])]
        o = flip[o]
    n_all = adjMat.n
    if n_all < 2:
        fast = np.zeros(2 * gaps)
    elif len(ids) == 0:
        rows = np.stack([layout.positions(new_id, sg == "-") for _i, sg in tags])
        fast = ctx.p2_score(rows, total)
    else:
        ctx.p2_set_arrangement(ids, rev)
        by_gap_rev = ctx.p2_score_insertions(new_id, total)             # [2*gap + (orientation == '-')]
        fast = np.array([by_gap_rev[2 * i + (1 if sg == "-" else 0)] for i, sg in tags])
    pieces = [layout.positions(int(i), int(r)) for i, r in zip(ids, rev)]

    def row_of(c):
        i, sg = tags[c]
        return np.concatenate(pieces[:i] + [layout.positions(new_id, sg == "-")] + pieces[i:])
    pick, bestCost = adjMat.first_strict_max(fast, 0., row_of)
    bestGap, bestOrient = tags[pick] if pick >= 0 else (0, "+")
    if gaps % 2 == 1:                                   # one flip per gap (OG:356)
        scaffToCheck.flipOrientation()
    if scaffToCheck.orientation != bestOrient:
        scaffToCheck.flipOrientation()
    orderedScaffs.insert(bestGap, scaffToCheck)
    return orderedScaffs, bestCost


def _insertion_job(orderedScaffolds, scaffoldList, matrix: GenomeMatrix):
    """(ids, rev, new_ids) for hicmi_p2_insert_all, or None when the whole-loop call does not apply (test
    doubles, score hooks, nothing left to add, a scaffold that was flipped before)."""
    layout = matrix.chrom
    if (layout is not None and _fused(matrix.ctx) and len(scaffoldList) > 0 and len(orderedScaffolds) > 0
            and layout.covers(orderedScaffolds) and layout.covers(scaffoldList)
            and all(s.orientation == "+" for s in scaffoldList)):
        ids, rev = layout.describe(orderedScaffolds)
        return ids, rev, [layout.sid[s.name] for s in scaffoldList]
    return None


def _insertion_result(ids, rev, orderedScaffolds, scaffoldList, matrix: GenomeMatrix):
    """Scaffold objects in the order / orientation hicmi_p2_insert_all returned; empties scaffoldList."""
    layout = matrix.chrom
    by_name = {s.name: s for s in orderedScaffolds + scaffoldList}
    del scaffoldList[:]
    ordered, _nodes = reorderScaffList([layout.names[i] for i in ids], ["-" if r else "+" for r in rev], by_name)
    return ordered


def orderRemainderScaffolds(orderedScaffolds, scaffoldList, orderDict, matrix: GenomeMatrix, binList):
    """OG:475-493 (a do-while: with nothing left to add, the last ordered scaffold is re-inserted)."""
    job = _insertion_job(orderedScaffolds, scaffoldList, matrix)
    if job is not None:
        ids, rev, bestCost = matrix.ctx.p2_insert_all(*job)
        return _insertion_result(ids, rev, orderedScaffolds, scaffoldList, matrix), bestCost
    while True:
        orderedScaffolds, scaffoldList = pullScaffolds(orderedScaffolds, scaffoldList, 1)
        adjMat, orderDict = giveNewAdjMat(matrix, orderedScaffolds, binList)
        newScaff = orderedScaffolds.pop(-1)
        orderedScaffolds, bestCost = checkAllScores(adjMat, orderDict, orderedScaffolds, newScaff)
        if len(scaffoldList) == 0:
            break
    return orderedScaffolds, bestCost


def scanOrdering(orderedScaffolds, scaffoldDict, orderDict, matrix: GenomeMatrix, binList, bestCost, scanScaffolds=5):
    """OG:495-549: slide a window of ``scanScaffolds`` scaffolds along the chromosome; every
    order/orientation of the window is scored on the WHOLE chromosome; repeat until a full pass
    brings no improvement."""
    adjMat, orderDict = giveNewAdjMat(matrix, orderedScaffolds, binList)
    total = adjMat.total()
    bestOrder = [s.name for s in orderedScaffolds]
    bestOrientation = [s.orientation for s in orderedScaffolds]
    roundNumber = 0
    w = scanScaffolds
    orders, orients = _enumeration(w)
    cur_fast = None                                     # fast score of the current arrangement
    if _fused(adjMat.ctx):
        layout = adjMat.layout
        layout.tables(w)
        ids, rev = layout.describe(orderedScaffolds)
        # the whole loop as one native call (the interpreter lock is free for the other chromosomes meanwhile)
        ids, rev, bestCost, cur_fast, roundNumber = adjMat.ctx.p2_scan_all(ids, rev, w, total, bestCost, cur_fast)
        for r in range(roundNumber):
            print("Working on round " + str(r + 1) + " of final step...")
        orderedScaffolds, _nodes = reorderScaffList([layout.names[i] for i in ids], ["-" if r else "+" for r in rev],
                                                    scaffoldDict)
        print("Sliding window conversion after " + str(roundNumber) + " rounds")
        print("Best cost at the end of the final step = " + str(bestCost))
        if _PROFILE:
            sys.stderr.write("[hicmi] part2 scan: %d scaffolds, %d rounds\n" % (len(ids), roundNumber))
        return orderedScaffolds, bestCost
    while True:
        improved = False
        print("Working on round " + str(roundNumber + 1) + " of final step...")
        for i in range(0, len(orderedScaffolds) - w + 1):
            if cur_fast is None:
                ids, rev = adjMat.layout.describe(orderedScaffolds)
                adjMat.ctx.p2_set_arrangement(ids, rev)
                cur_fast = adjMat.ctx.p2_arrangement_score(total)
            fast, row_of = _window_scores(adjMat, orderedScaffolds, i, w, known_fast=cur_fast)
            pick, bestCost = adjMat.first_strict_max(fast, bestCost, row_of)   # strict '>' vs the global best (OG:535)
            if pick >= 0:
                improved = True
                o, r = orders[pick // len(orients)], orients[pick % len(orients)]
                window = orderedScaffolds[i:i + w]
                names = [s.name for s in orderedScaffolds]
                outside = {s.name: s.orientation for s in orderedScaffolds}
                bestOrder = names[:i] + [window[j].name for j in o] + names[i + w:]
                bestOrientation = ([outside[nm] for nm in names[:i]] + list(r) + [outside[nm] for nm in names[i + w:]])
                cur_fast = float(fast[pick])
            orderedScaffolds, _nodes = reorderScaffList(bestOrder, bestOrientation, scaffoldDict)
        roundNumber += 1
        if not improved:
            break
    print("Sliding window conversion after " + str(roundNumber) + " rounds")
    print("Best cost at the end of the final step = " + str(bestCost))
    return orderedScaffolds, bestCost


def _startChromosome(chromGroup, matrix: GenomeMatrix, binList, nScaffolds=6, scanScaffolds=5):
    """OG:551-576: the selection, the brute-force order of the largest scaffolds; returns the state the
    insertion and scan phases continue from."""
    if nScaffolds >= 9:
        print("Number of initial scaffolds to order by brute force method is set too high... setting it to 8")
        nScaffolds = 8
    if scanScaffolds > nScaffolds:
        scanScaffolds = nScaffolds
    tm = [time.perf_counter()] if _PROFILE else None
    scaffoldList, scaffoldDict = initiateBinsAndScaffolds(chromGroup)
    if tm: tm.append(time.perf_counter())
    matrix.chrom = ChromosomeLayout(matrix, scaffoldList, binList)      # one selection for the whole chromosome
    if tm: tm.append(time.perf_counter())
    orderedScaffolds, scaffoldList = pullScaffolds([], scaffoldList, nScaffolds)
    adjMat, orderDict = giveNewAdjMat(matrix, orderedScaffolds, binList)
    if tm: tm.append(time.perf_counter())
    bfOrder, bfOrient, _bfScore = bruteForceBestScore(orderedScaffolds, scaffoldDict, adjMat, orderDict)
    if tm: tm.append(time.perf_counter())
    orderedScaffolds, _nodes = reorderScaffList(bfOrder, bfOrient, scaffoldDict)
    if tm:
        tm.append(time.perf_counter())
        sys.stderr.write("[hicmi] part2 start of a %d-bin chromosome (ms): scaffolds %.2f, layout + selection %.2f, sub-matrix view %.2f, "
                         "brute force %.2f, reorder %.2f\n" % ((len(chromGroup),) + tuple((b - a) * 1e3 for a, b in zip(tm, tm[1:]))))
    return {"ordered": orderedScaffolds, "rest": scaffoldList, "dict": scaffoldDict, "orderDict": orderDict,
            "nScaffolds": nScaffolds, "scanScaffolds": scanScaffolds}


def _start_all_applies(ctx):
    """Every chromosome's start phase in one native call (hicmi_p2_start_all) unless a test wants to see every fast score
    (SCORE_HOOK), the context is a test double without the call, or an A/B switch asks for the per-chromosome path."""
    return START_ALL and START_THREADS == 0 and SCORE_HOOK is None and hasattr(ctx, "p2_start_all")


def _uncaptured(fn, *args):
    """The ``capture`` of a plain run: what ``fn`` prints goes to stdout as it is."""
    return fn(*args), None


def _startOne(c, width, chromList, lane, binList):
    """One start job, chromosome ``c`` at brute-force width ``width``, by the per-chromosome calls."""
    print("#####################\n#####################")
    print("Working on Chr_" + str(c + 1) + "...")
    return _startChromosome(chromList[c], lane, binList, width, width)


def _startJobs(todo, chromList, lanes, binList, nScaffolds, jobs=None):
    """Host side of the batched start phase: per job of ``todo`` its scaffold grouping, its ChromosomeLayout (nothing
    issued to the device) and the job tuple of ``Context.p2_start_all`` - (context, selection, scaffold starts, scaffold
    lengths, ids of the scaffolds the brute force orders).  A job is a chromosome index at the width ``nScaffolds``
    (already clipped to 8), or, with ``jobs``, a key of it: ``jobs[key]`` = (chromosome index, width)."""
    prepared, out = {}, []
    for i in todo:
        c, width = (i, nScaffolds) if jobs is None else jobs[i]
        scaffoldList, scaffoldDict = initiateBinsAndScaffolds(chromList[c], quiet=True)
        layout = ChromosomeLayout(lanes[i], scaffoldList, binList, issue=False)
        orderedScaffolds, scaffoldList = pullScaffolds([], scaffoldList, min(width, 8))
        first_ids = [layout.sid[s.name] for s in orderedScaffolds]
        prepared[i] = (layout, orderedScaffolds, scaffoldList, scaffoldDict)
        out.append((lanes[i].ctx, layout.sel, layout.start, layout.length, first_ids))
    return prepared, out


def _started(c, width, scanScaffolds, lane, prepared, result):
    """What _startOne prints and returns, for a job whose native half hicmi_p2_start_all has done."""
    layout, orderedScaffolds, scaffoldList, scaffoldDict = prepared
    total, best, _bfScore, status = result
    print("#####################\n#####################")
    print("Working on Chr_" + str(c + 1) + "...")
    if width >= 9:
        print("Number of initial scaffolds to order by brute force method is set too high... setting it to 8")
    print("Scaffolds to order for this chromosome " + str(len(scaffoldDict)))
    lane.chrom = layout
    orderDict = _OrderDict(orderedScaffolds)
    names = [s.name for s in orderedScaffolds]
    k = len(names)
    orders, orients = _enumeration(k)
    if status == 1:                                  # OG:449: nothing is scored
        print("WARNING/ERROR - Zero contact values found between scaffolds assigned to chromosome group "
              + ",".join(str(e) for e in names))
        bfOrder, bfOrient = [names[j] for j in orders[0]], list(orients[0])
    else:
        print("Initial permutations to test " + str(len(orders) * len(orients)) + "...")
        layout._tables_k = k
        # the enumeration leaves every scaffold in the last candidate's orientation (OG:459)
        reorderScaffList([names[j] for j in orders[-1]], orients[-1], scaffoldDict)
        if best < 0:
            raise RuntimeError("no candidate order scored above 0 (the reference fails here too, OG:473 -> OG:576)")
        bfOrder, bfOrient = [names[j] for j in orders[best // len(orients)]], list(orients[best % len(orients)])
    orderedScaffolds, _nodes = reorderScaffList(bfOrder, bfOrient, scaffoldDict)
    return {"ordered": orderedScaffolds, "rest": scaffoldList, "dict": scaffoldDict, "orderDict": orderDict,
            "nScaffolds": min(width, 8), "scanScaffolds": min(scanScaffolds, width, 8)}


def _startAll(todo, chromList, lanes, binList, nScaffolds=6, scanScaffolds=5, jobs=None, capture=None):
    """_startOne for every job of ``todo`` (see _startJobs) with ONE native call: the same printed lines in the same order,
    the same state per job (the per-chromosome function stays the reference implementation of this one).  Returns
    {job: state}, or with ``capture`` {job: (state, the job's lines)}."""
    tm = [time.perf_counter()]
    prepared, calls = _startJobs(todo, chromList, lanes, binList, nScaffolds, jobs)
    tm.append(time.perf_counter())
    results = lanes[todo[0]].ctx.p2_start_all(calls, {k: _table_arrays(k) for k in {len(j[4]) for j in calls}}) if calls else []
    tm.append(time.perf_counter())
    call = capture or (lambda fn, *args: fn(*args))
    states = {}
    for i, result in zip(todo, results):
        c, width = (i, nScaffolds) if jobs is None else jobs[i]
        states[i] = call(_started, c, width, scanScaffolds, lanes[i], prepared[i], result)
    if _PROFILE:
        tm.append(time.perf_counter())
        sys.stderr.write("[hicmi] part2 start of %d chromosomes in one call (ms): scaffolds + flat arrays %.2f, native call %.2f, "
                         "reorder %.2f\n" % ((len(todo),) + tuple((b - a) * 1e3 for a, b in zip(tm, tm[1:]))))
    return states


def _scan_arranged_applies(ctx):
    return SCAN_ARRANGED and _fused(ctx) and hasattr(ctx, "p2_scan_arranged")


def _finishArranged(state, ids, rev, bestCost, matrix: GenomeMatrix):
    """_finishChromosome (OG:578-586) for a chromosome that is scanned, entered with the arrangement as the insertion
    queue returned it: set-up, total (OG:506) and rounds are one native call (hicmi_p2_scan_arranged), and the Scaffold
    objects are rebuilt once, after it.  The printed lines are those of _finishChromosome / scanOrdering."""
    print("BestCost at the end of first two steps " + str(bestCost))
    layout = matrix.chrom
    w = state["scanScaffolds"]
    orders, orients = _table_arrays(w)
    ids, rev, bestCost, roundNumber, _total = layout.ctx.p2_scan_arranged(ids, rev, w, orders, orients, bestCost)
    layout._tables_k = w
    for r in range(roundNumber):
        print("Working on round " + str(r + 1) + " of final step...")
    del state["rest"][:]
    orderedScaffolds, _nodes = reorderScaffList([layout.names[i] for i in ids], ["-" if r else "+" for r in rev], state["dict"])
    print("Sliding window conversion after " + str(roundNumber) + " rounds")
    print("Best cost at the end of the final step = " + str(bestCost))
    if _PROFILE:
        sys.stderr.write("[hicmi] part2 scan: %d scaffolds, %d rounds\n" % (len(ids), roundNumber))
    print("Final ordering...")
    for s in orderedScaffolds:
        print(s.name, s.orientation)
    orderChromosome.last_cost = bestCost
    return orderedScaffolds


def _finishChromosome(state, orderedScaffolds, bestCost, matrix: GenomeMatrix, binList):
    """OG:578-586: the sliding-window rounds and the final listing."""
    print("BestCost at the end of first two steps " + str(bestCost))
    if len(orderedScaffolds) > state["nScaffolds"]:
        orderedScaffolds, bestCost = scanOrdering(orderedScaffolds, state["dict"], state["orderDict"], matrix, binList,
                                                  bestCost, scanScaffolds=state["scanScaffolds"])
    print("Final ordering...")
    for s in orderedScaffolds:
        print(s.name, s.orientation)
    orderChromosome.last_cost = bestCost
    return orderedScaffolds


def orderChromosome(chromGroup, matrix: GenomeMatrix, binList, nScaffolds=6, scanScaffolds=5):
    """OG:551-586."""
    state = _startChromosome(chromGroup, matrix, binList, nScaffolds, scanScaffolds)
    orderedScaffolds, bestCost = orderRemainderScaffolds(state["ordered"], state["rest"], state["orderDict"], matrix,
                                                         binList)
    return _finishChromosome(state, orderedScaffolds, bestCost, matrix, binList)


def _finishJob(state, after, scanScaffolds, lane, binList, own):
    """One scan job from where its start job's insertion ended - ``after`` is (ids, rev, bestCost) as the lock step returned
    them, or (Scaffold objects, bestCost) from orderRemainderScaffolds: the sliding-window rounds, the final listing and the
    chromosome's text in the two output files, formatted here, beside the other lanes' native scan calls.  ``own``: the start
    job has other scans too, and a scan flips Scaffold objects in place, so this one works on copies."""
    if own:
        mine = {name: s.copy() for name, s in state["dict"].items()}
        state = dict(state, dict=mine, **{k: [mine[s.name] for s in state[k]] for k in ("ordered", "rest")})
        if len(after) == 2:
            after = ([mine[s.name] for s in after[0]], after[1])
    state = dict(state, scanScaffolds=state["nScaffolds"] if scanScaffolds is None else min(scanScaffolds, state["nScaffolds"]))
    if len(after) == 3 and len(after[0]) > state["nScaffolds"] and _scan_arranged_applies(lane.ctx):
        # scanned: the insertion's ids / rev go straight back into native code (which works on copies of them), Scaffold
        # objects come afterwards
        res = _finishArranged(state, after[0], after[1], after[2], lane)
    else:
        if len(after) == 3:
            after = (_insertion_result(after[0], after[1], state["ordered"], state["rest"], lane), after[2])
        res = _finishChromosome(state, after[0], after[1], lane, binList)
    return res, (_scaffold_lines(res), _bin_rows(res))


def orderJobs(matrix: GenomeMatrix, chromList, binList, starts, scans, workers, capture=_uncaptured, on_native_phase=None):
    """Part 2's three phases over any set of jobs: a -part2 run is one start and one scan job per chromosome, a sweep
    (sweepPart2.py) shares start jobs between settings.

    ``starts``: [(chromosome index, brute-force width)] - selection, brute force and insertion, each job on a lane of its
    own.  ``scans``: [(index into starts, scanScaffolds or None for the width)] - the sliding-window rounds (when the
    chromosome has more scaffolds than the width) and the final listing; the scans of one start job run one after the other
    on its lane.  Phases: (1) every start job, on this thread, in one native call where that applies; (2) every insertion loop in
    lock step, decided on the device - one queue of launches serving all of them (hicmi_p2_insert_all_multi); (3) the scans
    on ``workers`` threads.  A context without worker lanes or the lock step (a test double; SCORE_HOOK) runs the same
    steps one start job after the other on the one context.

    ``capture(fn, *args) -> (result, lines)`` wraps everything that prints a job's lines.  Returns
    ([(lane, layout, lines) per start job], [((scaffolds, (_scaffold_lines, _bin_rows)), lines) per scan job])."""
    t0 = time.perf_counter()
    matrix.bin_index(binList)
    ctx = matrix.ctx
    lockstep = SCORE_HOOK is None and hasattr(ctx, "workers") and hasattr(ctx, "p2_insert_all_multi")
    lanes = matrix.lanes(len(starts)) if lockstep else [matrix] * len(starts)
    todo = sorted(range(len(starts)), key=lambda j: -len(chromList[starts[j][0]]))             # largest first
    by_start = {}
    for s, (j, _w) in enumerate(scans):
        by_start.setdefault(j, []).append(s)
    started, raw, finished = [None] * len(starts), {}, [None] * len(scans)
    marks = [time.perf_counter()]
    if _PROFILE:
        sys.stderr.write("[hicmi] part2 set-up (bin index, one context per chromosome): %.1f ms\n" % ((marks[0] - t0) * 1e3))

    def start(j):
        state, lines = capture(_startOne, starts[j][0], starts[j][1], chromList, lanes[j], binList)
        started[j] = (state, lanes[j].chrom, lines)

    def finish(j):
        state, lane = started[j][0], lanes[j]
        after = raw.get(j)
        if after is None:                                        # e.g. nothing left to add (OG:475-493)
            after = orderRemainderScaffolds(state["ordered"], state["rest"], state["orderDict"], lane, binList)
        for s in by_start.get(j, ()):
            tf = time.perf_counter()
            finished[s] = capture(_finishJob, state, after, scans[s][1], lane, binList, len(by_start[j]) > 1)
            if _PROFILE:
                c = starts[j][0]
                sys.stderr.write("[hicmi] part2 scan of chromosome %d (%d bins): start +%.1f ms, %.1f ms\n"
                                 % (c + 1, len(chromList[c]), (tf - marks[-1]) * 1e3, (time.perf_counter() - tf) * 1e3))

    if not lockstep:
        for j in range(len(starts)):
            start(j)
            finish(j)
    else:
        # the start phase runs on THIS thread, one job after the other: it is half interpreter work and half short native
        # calls, and threads that hand the interpreter lock to each other at every one of those calls took 12-14 ms (16k) /
        # 22-24 ms (32k) where the plain loop takes 7.7 / 13.5 ms
        if _start_all_applies(ctx):
            # ... and its native half as ONE call over all jobs (hicmi_p2_start_all): their kernels are queued behind each
            # other on their own streams and waited for phase by phase
            for j, (state, lines) in _startAll(todo, chromList, lanes, binList, jobs=starts, capture=capture).items():
                started[j] = (state, lanes[j].chrom, lines)
        elif START_THREADS > 0:
            with ThreadPoolExecutor(max_workers=START_THREADS) as starters:
                list(starters.map(start, todo))
        else:
            for j in todo:
                start(j)
        marks.append(time.perf_counter())
        jobs, job_of = [], []
        for j in todo:
            job = _insertion_job(started[j][0]["ordered"], started[j][0]["rest"], lanes[j])
            if job is not None:
                jobs.append((lanes[j].ctx,) + job)
                job_of.append(j)
        if on_native_phase is not None:
            on_native_phase()                     # a long native call follows: background Python work may take the GIL
        raw.update(zip(job_of, ctx.p2_insert_all_multi(jobs)))     # (turned into scaffold lists by the scan threads)
        marks.append(time.perf_counter())
        with ThreadPoolExecutor(max_workers=max(1, min(workers, len(by_start)))) as pool:
            list(pool.map(finish, todo))
        marks.append(time.perf_counter())
        if _PROFILE:
            sys.stderr.write("[hicmi] part2 lock step: start %.1f ms, insertion %.1f ms (%d chromosomes), scan %.1f ms\n"
                             % ((marks[1] - marks[0]) * 1e3, (marks[2] - marks[1]) * 1e3, len(jobs),
                                (marks[3] - marks[2]) * 1e3))
    return [(lanes[j], layout, lines) for j, (_state, layout, lines) in enumerate(started)], finished


def chromosomesOfRank(chromList, rank, world):
    """The chromosomes one rank orders when a single map is spread over ``world`` processes: largest first, each
    to the rank with the least work so far (work ~ bins squared, the size of the chromosome's sub-matrix; ties go
    to the lowest rank).  Every rank computes the same deal from the same group file - no exchange needed."""
    load = [0] * world
    mine = []
    for i in sorted(range(len(chromList)), key=lambda i: (-len(chromList[i]), i)):
        r = min(range(world), key=lambda k: (load[k], k))
        load[r] += len(chromList[i]) ** 2
        if r == rank:
            mine.append(i)
    return sorted(mine)


def orderGenome(matrix: GenomeMatrix, chromList, binList, resolution, nScaffolds=6, scanScaffolds=5, plotChrom=True,
                showPlot=True, savePlotDir=False, plotTitleSuffix=False, shard=None, on_native_phase=None):
    """OG:591-628.  Chromosomes are independent (OG:608-612), so they are ordered concurrently:
    one host thread + one libhicmi context (own HIP stream, own scratch) per chromosome in flight,
    all reading the same device-resident contact matrix.  Results are collected in file order.
    The per-chromosome figures (OG:615-622) are drawn afterwards from the device-resident matrix.

    ``shard=(rank, world)``: one map over several GPUs.  Every rank holds the map, orders only the
    chromosomes ``chromosomesOfRank`` deals to it and draws their figures; one object all-gather of the ordered
    scaffold lists (names, orientations, bin IDs: a few KB) gives every rank the whole genome order."""
    t0 = time.time()
    t0p = time.perf_counter()
    pieces = None                                          # per chromosome: its text in the two output files, when formatted on the way
    orderGenome.file_text = None
    indices = list(range(len(chromList))) if shard is None else chromosomesOfRank(chromList, shard[0], shard[1])
    n_workers = 1 if SCORE_HOOK is not None else max(1, min(WORKERS, len(indices)))

    def one(i, m):
        print("#####################\n#####################")
        print("Working on Chr_" + str(i + 1) + "...")
        if not _PROFILE:
            return orderChromosome(chromList[i], m, binList, nScaffolds=nScaffolds, scanScaffolds=scanScaffolds)
        ts = time.perf_counter()
        res = orderChromosome(chromList[i], m, binList, nScaffolds=nScaffolds, scanScaffolds=scanScaffolds)
        te = time.perf_counter()
        sys.stderr.write("[hicmi] part2 chr %d: %d bins, %d scaffolds, start %.1f ms, %.1f ms\n"
                         % (i + 1, len(chromList[i]), len(res), (ts - t0p) * 1e3, (te - ts) * 1e3))
        return res

    if n_workers == 1 or not hasattr(matrix.ctx, "workers"):
        done = {i: one(i, matrix) for i in indices}
    elif LOCKSTEP and hasattr(matrix.ctx, "p2_insert_all_multi"):
        # one start job and one scan job per chromosome, all in flight together (orderJobs)
        _started_jobs, finished = orderJobs(matrix, chromList, binList, [(i, nScaffolds) for i in indices],
                                            [(k, scanScaffolds) for k in range(len(indices))], n_workers,
                                            on_native_phase=on_native_phase)
        done = {i: res for i, ((res, _text), _lines) in zip(indices, finished)}
        if shard is None:
            pieces = {i: text for i, ((_res, text), _lines) in zip(indices, finished)}
    else:
        matrix.bin_index(binList)
        free = matrix.lanes(n_workers)
        todo = sorted(indices, key=lambda i: -len(chromList[i]))                    # largest first

        def run(i):
            m = free.pop()
            try:
                return i, one(i, m)
            finally:
                free.append(m)
        with ThreadPoolExecutor(max_workers=n_workers) as pool:
            done = dict(pool.map(run, todo))
    if shard is not None:
        from . import dist
        done = dist.gather_results(done)
    fullGenomeOrder = [done[i] for i in range(len(chromList))]
    if pieces is not None and len(pieces) == len(chromList):
        orderGenome.file_text = [pieces[i] for i in range(len(chromList))]
    print("RunTime for total genome = " + str(time.time() - t0))
    if plotChrom is True and plotModule.plots_enabled(savePlotDir):
        # OG:615-622: one figure per chromosome.  The device reductions run here one after the other (a context
        # is not thread-safe), the drawing and PNG encoding on worker threads.
        where = matrix.bin_index(binList)
        todo = []
        for i in indices:
            rows = [where[b] for s in fullGenomeOrder[i] for b in s.binList]
            if len(rows) == 0:
                continue
            img = plotModule.DeviceImage(matrix.ctx, 0, rows)
            img.prefetch([1, 98], plotModule.figure_pixels(len(rows), 24, 24))
            todo.append((i, img))

        def draw(item):
            i, img = item
            chrName = "Chr_" + str(i + 1)
            plotModule.plotContactMap(img, resolution=resolution, tickCount=11, highlightChroms=False, wInches=24,
                                      hInches=24, lP=1, hP=98, reverseColorMap='', showPlot=False,
                                      savePlot=savePlotDir + "/" + chrName + ".png", title=chrName,
                                      titleSuffix=plotTitleSuffix)
        with ThreadPoolExecutor(max_workers=max(1, min(8, len(todo)))) as pool:
            list(pool.map(draw, todo))
        print("RunTime for total genome with plotting and saving .pngs = " + str(time.time() - t0))
    return fullGenomeOrder


def _scaffold_lines(group):
    """A chromosome's lines of the scaffold-order file (OG:638-641)."""
    return "".join([s.name + "\t" + s.orientation + "\n" for s in group])


def _bin_rows(scaffoldList):
    """Newline-PREFIXED ``scaffold<TAB>bin`` rows (OG:654-657) and how many."""
    rows, n_rows = [], 0
    for s in scaffoldList:
        if len(s.binList):
            head = "\n" + s.name + "\t"
            rows.append(head + head.join(map(str, s.binList)))
            n_rows += len(s.binList)
    return "".join(rows), n_rows


def writeScaffoldOrderingsToFile(sOrderings, outFile, lines=None):
    """OG:630-644.  ``lines``: per group, its lines already formatted (_scaffold_lines)."""
    text = []
    for k, group in enumerate(sOrderings):
        text.append("### Chromosome grouping " + str(k + 1) + " ###\n")
        text.append(lines[k] if lines is not None else _scaffold_lines(group))
    with open(outFile, "w") as fh:
        fh.write("".join(text))
    print("Chromosome groups written to file " + str(len(sOrderings)))
    print("Scaffolds written to file " + str(sum(len(g) for g in sOrderings)))


def writeBinIDsOrderingToFile(scaffoldList, outFile, rows=None):
    """OG:646-660: header line, then newline-PREFIXED rows (no trailing newline).  ``rows``: (text, count) pieces that
    together are _bin_rows(scaffoldList)."""
    if rows is None:
        rows = [_bin_rows(scaffoldList)]
    with open(outFile, "w") as fh:
        fh.write("#ScaffoldID\tHiCPro-BinID" + "".join(r[0] for r in rows))
    print("BinIDs written to file " + str(sum(r[1] for r in rows)))


# ---- placement support of a finished ordering -----------------------------------------
SUPPORT_DIRECT_BYTES = 64 << 20        # HICMI_P2_SUPPORT_DIRECT=1: bytes of materialised candidate rows resident at a time


def scaffoldsFromOrderFile(chromList, chromosomeOrderFile):
    """A chromosomeOrderFile (this project's or the reference's) back as lists of Scaffold objects: chromosome i of the
    order file takes its bins from group i of ``chromList`` (readChromsFromFile of the group file)."""
    groups, cur = [], None
    with open(chromosomeOrderFile) as fh:
        for line in fh:
            line = line.rstrip("\r\n")
            if not line:
                continue
            if line[0] == "#":
                cur = []
                groups.append(cur)
            else:
                if cur is None:
                    raise ValueError(chromosomeOrderFile + ": a scaffold line before the first chromosome header")
                cols = line.split("\t")
                if len(cols) < 2 or cols[1] not in ("+", "-"):
                    raise ValueError(chromosomeOrderFile + ": expected 'scaffold<TAB>+/-', found " + repr(line))
                cur.append((cols[0], cols[1]))
    if len(groups) != len(chromList):
        raise ValueError("%s lists %d chromosomes, the group file %d" % (chromosomeOrderFile, len(groups), len(chromList)))
    out = []
    for i, (group, chrom) in enumerate(zip(groups, chromList)):
        bins_of = {}
        for bin_id, name in chrom:
            bins_of.setdefault(name, []).append(bin_id)
        if sorted(bins_of) != sorted(name for name, _o in group):
            raise ValueError("chromosome %d: the order file and the group file do not list the same scaffolds" % (i + 1))
        scaffs = []
        for name, orient in group:
            sc = Scaffold(name, sorted(bins_of[name]), "+")
            if orient == "-":
                sc.flipOrientation()
            scaffs.append(sc)
        out.append(scaffs)
    return out


def _support_row(layout, ids, rev, j, g, r):
    """Bin order (selection indices) of "the arrangement without scaffold j, j put back at gap g in orientation r"."""
    oi = [int(v) for k, v in enumerate(ids) if k != j]
    orr = [int(v) for k, v in enumerate(rev) if k != j]
    oi.insert(g, int(ids[j]))
    orr.insert(g, int(r))
    return layout.node_row(oi, orr)


def support_counts(lengths, rev):
    """(S, S, 2) mask of the candidates that compete for a scaffold's best move: those whose bin order differs from the
    arrangement's - not (g = j, r = its orientation) - and, of a one-bin scaffold, only '+' away from its own gap ('-'
    is the same bin order and comes second in enumeration order, so it can never be a strict maximum).  A chromosome
    of one scaffold has no other placement (its flip is the whole chromosome read backwards)."""
    S = len(lengths)
    m = np.ones((S, S, 2), dtype=bool)
    if S == 1:
        m[:] = False
    for j in range(S):
        if lengths[j] == 1:
            m[j, :, 1] = False
            m[j, j, :] = False
        else:
            m[j, j, int(rev[j])] = False
    return m


def support_summary(table, lengths, rev):
    """What hicmi_p2_support returns as ``best`` from a table of scores: per scaffold [2 g + r of the first maximum over
    support_counts, or -1; how many counted candidates lie within NEAR_TOP of it]."""
    S = len(lengths)
    counts = support_counts(lengths, rev).reshape(S, 2 * S)
    flat = np.asarray(table, dtype=np.float64).reshape(S, 2 * S)
    out = np.zeros((S, 2), np.int32)
    for j in range(S):
        ok = counts[j] & np.isfinite(flat[j])
        if not ok.any():
            out[j] = (-1, 0)
            continue
        v = np.where(ok, flat[j], -np.inf)
        top = float(v.max())
        out[j] = (int(np.argmax(v)), int(np.count_nonzero(v >= top - abs(top) * NEAR_TOP)))
    return out


def _score_rows(layout, total, flat, row_of):
    """flat[c] = hicmi_p2_score of candidate c's materialised bin order ``row_of(c)``, at most SUPPORT_DIRECT_BYTES of
    rows at a time: the table of the two DIRECT paths."""
    per = max(1, SUPPORT_DIRECT_BYTES // (4 * layout.n))
    for c0 in range(0, len(flat), per):
        rows = np.stack([row_of(c) for c in range(c0, min(c0 + per, len(flat)))]).astype(np.int32)
        flat[c0:c0 + len(rows)] = layout.ctx.p2_score(rows, total)


def _support_direct(layout, ids, rev, total):
    """A/B path (HICMI_P2_SUPPORT_DIRECT=1): the same table from hicmi_p2_score on every candidate's materialised bin
    order, at most SUPPORT_DIRECT_BYTES of rows at a time."""
    S = len(ids)
    table = np.zeros((S, S, 2))
    if layout.n >= 2 and total > 0:
        _score_rows(layout, total, table.reshape(-1), lambda c: _support_row(layout, ids, rev, c // (2 * S), (c // 2) % S, c % 2))
        return table, support_summary(table, [layout.length[int(i)] for i in ids], rev)
    return table, np.tile(np.array([-1, 0], np.int32), (S, 1))


def _literal_rows(layout, rows, total):
    """hicmi_p2_score_exact of explicit bin orders, at most SUPPORT_DIRECT_BYTES of rows per call."""
    per = max(1, SUPPORT_DIRECT_BYTES // (4 * max(1, layout.n)))
    out = [layout.ctx.p2_score_exact(np.stack(rows[i:i + per]).astype(np.int32), total) for i in range(0, len(rows), per)]
    return np.concatenate(out) if out else np.zeros(0)


def _decide_near(flat, counts, pick, row_of, layout, total):
    """A pick with rivals within NEAR_TOP (a near count above 1) decided: ``flat`` are the scaffold's closed-form scores
    and ``counts`` the candidates that compete; the table only ranks, so the rivals' bin orders ``row_of(c)`` are scored
    literally (hicmi_p2_score_exact) and the first strict maximum in enumeration order is the pick."""
    top = float(flat[pick])
    near = np.flatnonzero(counts & np.isfinite(flat) & (flat >= top - abs(top) * NEAR_TOP))
    top_lit = -math.inf
    for c, v in zip(near, _literal_rows(layout, [row_of(int(c)) for c in near], total)):
        if v > top_lit:
            pick, top_lit = int(c), float(v)
    return pick


def _support_one(layout, ids, rev, total, table, best):
    """One chromosome's result from its table: score0, flip / best columns and verdicts (the picks: _decide_near).
    The reported deltas are literal scores too - of the arrangement, each in-place flip and each best move, one
    call - so that they do not depend on how the table was computed."""
    S = len(ids)
    lengths = [layout.length[int(i)] for i in ids]
    live = layout.n >= 2 and total > 0
    counts = support_counts(lengths, rev).reshape(S, 2 * S)
    flat = table.reshape(S, 2 * S)
    picks = [int(best[j][0]) if live else -1 for j in range(S)]
    for j in range(S):
        if picks[j] >= 0 and int(best[j][1]) > 1:
            picks[j] = _decide_near(flat[j], counts[j], picks[j], lambda c: _support_row(layout, ids, rev, j, c // 2, c % 2),
                                    layout, total)
    flips = [j for j in range(S) if live and lengths[j] > 1 and S > 1]
    moves = [j for j in range(S) if picks[j] >= 0]
    lit = _literal_rows(layout, [layout.node_row(ids, rev)]
                        + [_support_row(layout, ids, rev, j, j, 1 - int(rev[j])) for j in flips]
                        + [_support_row(layout, ids, rev, j, picks[j] // 2, picks[j] % 2) for j in moves], total) if live else [0.0]
    score0 = float(lit[0])
    # a one-bin scaffold reads the same both ways, and a lone scaffold's flip is the chromosome read backwards: 0.0
    flip_of = dict(zip(flips, (float(v) - score0 for v in lit[1:1 + len(flips)])))
    move_of = dict(zip(moves, (float(v) - score0 for v in lit[1 + len(flips):])))
    rows = []
    for j in range(S):
        flip, delta = flip_of.get(j, 0.0), move_of.get(j)
        gap, orient = (None, None) if delta is None else (picks[j] // 2, "-" if picks[j] % 2 else "+")
        verdict = "improvable" if delta is not None and delta > 0 else ("orientation_open" if flip == 0 else "supported")
        rows.append({"bins": lengths[j], "flip_delta": flip, "best_gap": gap, "best_orientation": orient,
                     "best_delta": delta, "verdict": verdict})
    return {"score0": score0, "total": total, "table": table, "rows": rows}


def _layout_jobs(lanes, orderedChromosomes, binList, chromList):
    """The chromosomes of a finished ordering, len(lanes) at a time, each selected on its lane in orderChromosome's layout
    order (``chromList[k]``, the group file's rows, fixes it; without it the scaffolds are taken largest first in
    arrangement order): lists of (layout, ids, rev, total of the layout, scaffolds in arrangement order)."""
    for c0 in range(0, len(orderedChromosomes), len(lanes)):
        jobs = []
        for lane, k in zip(lanes, range(c0, min(c0 + len(lanes), len(orderedChromosomes)))):
            group = orderedChromosomes[k]
            if chromList is not None:
                by_name = {s.name: s for s in group}
                order = [by_name[s.name] for s in _layoutScaffolds(chromList[k])]
            else:
                order = sorted(group, key=lambda s: len(s.binList), reverse=True)
            layout = lane.chrom = ChromosomeLayout(lane, order, binList)
            total = layout.whole_total()
            ids, rev = layout.describe(group)
            jobs.append((layout, ids, rev, total, group))
        yield jobs


def _table_report(matrix, orderedChromosomes, binList, chromList, kind, direct_fn, job_of, extra, one, switch=None):
    """The driver of placementSupport (``kind`` "support"), breakSupport ("breaks") and inversionSupport ("inversions",
    whose switch is spelt HICMI_P2_INVERT_DIRECT: ``switch``): every chromosome's (table, best)
    from HICMI_P2_<KIND>_DIRECT=1's ``direct_fn(layout, ids, rev, total)``, else from one ctx.p2_<kind>_multi call per
    round of lanes, else (a context without lanes, or SCORE_HOOK) from ctx.p2_<kind> one by one - ``job_of(layout, ids,
    rev, total)``: a job's arguments after the context, ``extra``: the call's arguments after the jobs - and from those
    ``one(layout, ids, rev, total, table, best, group)``: the chromosome's result, here given its names and orientations."""
    ctx = matrix.ctx
    matrix.bin_index(binList)
    direct = os.environ.get(switch or "HICMI_P2_%s_DIRECT" % kind.upper(), "") not in ("", "0")
    multi = not direct and SCORE_HOOK is None and hasattr(ctx, "workers") and hasattr(ctx, "p2_%s_multi" % kind)
    lanes = matrix.lanes(len(orderedChromosomes)) if multi and len(orderedChromosomes) > 1 else [matrix]
    out = []
    for jobs in _layout_jobs(lanes, orderedChromosomes, binList, chromList):
        if direct:
            tables = [direct_fn(layout, ids, rev, total) for layout, ids, rev, total, _g in jobs]
        elif multi:
            tables = getattr(ctx, "p2_%s_multi" % kind)([(layout.ctx,) + job_of(layout, ids, rev, total)
                                                         for layout, ids, rev, total, _g in jobs], *extra)
        else:
            tables = [getattr(layout.ctx, "p2_" + kind)(*(job_of(layout, ids, rev, total) + extra))
                      for layout, ids, rev, total, _g in jobs]
        for (layout, ids, rev, total, group), (table, best) in zip(jobs, tables):
            res = one(layout, ids, rev, total, np.asarray(table), best, group)
            res["names"] = [s.name for s in group]
            res["orientations"] = [s.orientation for s in group]
            out.append(res)
    return out


def placementSupport(matrix: GenomeMatrix, orderedChromosomes, binList, chromList=None):
    """How well the map supports a finished ordering: every scaffold of every chromosome is taken out of its
    chromosome's arrangement and put back at every gap in both orientations (include/hicmi.h,
    hicmi_p2_support).  Returns one dict per chromosome: 'score0' (literal objective of the arrangement), 'total',
    'table' (S x S x 2 scores: left-out scaffold, gap of the arrangement without it, '+'/'-'), 'names', 'orientations'
    and 'rows' (per scaffold in arrangement order: bins, flip_delta, best_gap, best_orientation, best_delta, verdict).

    All scores of a chromosome are under ONE total, that of its selection in layout order with every scaffold '+', the
    layout being orderChromosome's: ``chromList[i]`` (the group file's rows) fixes it; without it the scaffolds are
    taken largest first in arrangement order.  On the device all chromosomes go through one hicmi_p2_support_multi
    call, one context each; HICMI_P2_SUPPORT_DIRECT=1 scores materialised candidates with hicmi_p2_score instead."""
    return _table_report(matrix, orderedChromosomes, binList, chromList, "support", _support_direct,
                         lambda layout, ids, rev, total: (ids, rev, total), (),
                         lambda layout, ids, rev, total, table, best, group: _support_one(layout, ids, rev, total, table, best))


def _layoutScaffolds(nodeList):
    """initiateBinsAndScaffolds' scaffold list (the layout order of orderChromosome) without its printed line."""
    bins_of = {}
    for bin_id, name in nodeList:
        bins_of.setdefault(name, []).append(bin_id)
    return sorted((Scaffold(name, sorted(b), "+") for name, b in bins_of.items()), key=lambda s: len(s.binList),
                  reverse=True)


def _support_text(v):
    return "NA" if v is None else (repr(v) if isinstance(v, float) else str(v))


def placementSupportText(results):
    """The report: per chromosome ``### Chromosome grouping i ### score0``, then one tab-separated line per scaffold in
    arrangement order: scaffold, orientation, bins, flip_delta, best_gap, best_orientation, best_delta, verdict.  Floats
    are written with repr; a chromosome of one scaffold has no other placement: NA."""
    text = []
    for k, res in enumerate(results):
        text.append("### Chromosome grouping " + str(k + 1) + " ### " + repr(res["score0"]) + "\n")
        for name, orient, row in zip(res["names"], res["orientations"], res["rows"]):
            text.append("\t".join([name, orient] + [_support_text(row[key]) for key in
                                                    ("bins", "flip_delta", "best_gap", "best_orientation", "best_delta",
                                                     "verdict")]) + "\n")
    return "".join(text)


def writePlacementSupportToFile(results, outFile, fullDir=None):
    """placementSupportText to ``outFile``; ``fullDir``: also each chromosome's S x 2S table as ``Chr_i.support.tsv``
    (row = left-out scaffold, columns = gap0+, gap0-, gap1+, ...)."""
    with open(outFile, "w") as fh:
        fh.write(placementSupportText(results))
    if fullDir:
        os.makedirs(fullDir, exist_ok=True)
        for k, res in enumerate(results):
            S = len(res["names"])
            with open(os.path.join(fullDir, "Chr_%d.support.tsv" % (k + 1)), "w") as fh:
                fh.write("\t".join(["scaffold"] + ["gap%d%s" % (g, o) for g in range(S) for o in "+-"]) + "\n")
                for name, line in zip(res["names"], np.asarray(res["table"]).reshape(S, 2 * S)):
                    fh.write("\t".join([name] + [repr(float(v)) for v in line]) + "\n")
    print("Placement support written for scaffolds " + str(sum(len(r["rows"]) for r in results)))


# ---- break support of a finished ordering ---------------------------------------------
BREAK_MOVES = ("as_is", "flip_right", "flip_left", "flip_both", "swap", "swap_flip_right", "swap_flip_left",
               "swap_flip_both")       # candidate k = 4 w + 2 x + y: pieces swapped, left piece reversed, right piece reversed


def _break_row(row0, B, L, p, k):
    """Bin order of candidate k of the cut after the first p of the L positions from B of ``row0``."""
    P, Q = row0[B:B + p], row0[B + p:B + L]
    if k & 2:
        P = P[::-1]
    if k & 1:
        Q = Q[::-1]
    return np.concatenate([row0[:B], Q, P, row0[B + L:]] if k & 4 else [row0[:B], P, Q, row0[B + L:]])


def break_counts(L, minPiece=1):
    """(L - 1, 8) mask of the candidates that compete for a scaffold's best break: both pieces have ``minPiece`` bins,
    and the bin order differs from the arrangement's, from the in-place whole flip's and from every earlier candidate's
    of the same cut (include/hicmi.h, hicmi_p2_breaks)."""
    m = np.zeros((max(L - 1, 0), 8), dtype=bool)
    for p in range(1, L):
        q = L - p
        if p < minPiece or q < minPiece:
            continue
        for k in range(1, 7):
            if (k & 2 and p == 1) or (k & 1 and q == 1):
                continue
            if (k == 5 and p == 1) or (k == 6 and q == 1) or (k == 4 and p == 1 and q == 1):
                continue
            m[p - 1, k] = True
    return m


def break_summary(block, L, minPiece=1):
    """What hicmi_p2_breaks returns as a scaffold's ``best`` from its (L - 1) x 8 block of scores: [8 (p - 1) + k of the
    first maximum over break_counts, or -1; how many competing candidates lie within NEAR_TOP of it]."""
    ok = (break_counts(L, minPiece) & np.isfinite(block)).reshape(-1)
    if not ok.any():
        return -1, 0
    v = np.where(ok, np.asarray(block, dtype=np.float64).reshape(-1), -np.inf)
    top = float(v.max())
    return int(np.argmax(v)), int(np.count_nonzero(v >= top - abs(top) * NEAR_TOP))


def _break_offsets(lengths):
    """First table row of every scaffold's (L - 1) x 8 block, and the number of rows."""
    off, at = [], 0
    for ln in lengths:
        off.append(at)
        at += max(ln - 1, 0)
    return off, at


def _breaks_direct(layout, ids, rev, total, minPiece):
    """A/B path (HICMI_P2_BREAKS_DIRECT=1): the same table from hicmi_p2_score on every candidate's materialised bin
    order, at most SUPPORT_DIRECT_BYTES of rows at a time."""
    lengths = [layout.length[int(i)] for i in ids]
    off, n_rows = _break_offsets(lengths)
    table = np.zeros((n_rows, 8))
    best = np.tile(np.array([-1, 0], np.int32), (len(ids), 1))
    if layout.n < 2 or not total > 0:
        return table, best
    row0 = layout.node_row(ids, rev)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    cands = [(int(starts[j]), L, p, k) for j, L in enumerate(lengths) for p in range(1, L) for k in range(8)]
    _score_rows(layout, total, table.reshape(-1), lambda c: _break_row(row0, *cands[c]))
    for j, L in enumerate(lengths):
        best[j] = break_summary(table[off[j]:off[j] + L - 1], L, minPiece)
    return table, best


def _breaks_one(layout, ids, rev, total, table, best, group, minPiece):
    """One chromosome's result from its table: score0, the best break of every scaffold and the verdicts (the picks:
    _decide_near).  The reported floats are literal scores too - the arrangement and every
    best break of the chromosome in one call - so that they do not depend on how the table was computed."""
    S = len(ids)
    lengths = [layout.length[int(i)] for i in ids]
    off, _n = _break_offsets(lengths)
    starts = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    live = layout.n >= 2 and total > 0
    row0 = layout.node_row(ids, rev)
    nears = [int(best[j][1]) if live else 0 for j in range(S)]
    picks = [int(best[j][0]) if live else -1 for j in range(S)]
    for j, L in enumerate(lengths):
        if picks[j] >= 0 and nears[j] > 1:
            picks[j] = _decide_near(table[off[j]:off[j] + L - 1].reshape(-1), break_counts(L, minPiece).reshape(-1), picks[j],
                                    lambda c: _break_row(row0, int(starts[j]), L, c // 8 + 1, c % 8), layout, total)
    moves = [j for j in range(S) if picks[j] >= 0]
    lit = _literal_rows(layout, [row0] + [_break_row(row0, int(starts[j]), lengths[j], picks[j] // 8 + 1, picks[j] % 8)
                                          for j in moves], total) if live else [0.0]
    score0 = float(lit[0])
    delta_of = dict(zip(moves, (float(v) - score0 for v in lit[1:])))
    rows = []
    for j in range(S):
        delta, L = delta_of.get(j), lengths[j]
        if delta is None:
            cut = after = move = gain = None
            verdict = "NA"
        else:
            p = picks[j] // 8 + 1
            cut = L - p if rev[j] else p                  # the scaffold's own bins before the cut, '+' direction
            after = sorted(group[j].binList)[cut - 1]
            move = BREAK_MOVES[picks[j] % 8]
            gain = delta / score0
            verdict = "breakable" if delta > 0 else "intact"
        rows.append({"bins": L, "best_cut": cut, "cut_after_bin": after, "best_move": move, "best_delta": delta,
                     "gain": gain, "verdict": verdict, "near": nears[j]})
    return {"score0": score0, "total": total, "table": table, "offsets": off, "rows": rows, "minPiece": minPiece}


def breakSupport(matrix: GenomeMatrix, orderedChromosomes, binList, chromList=None, minPiece=1):
    """Where the map would rather have a scaffold cut: every scaffold of every chromosome is cut between every two of
    its bins and the two pieces are swapped and / or reversed in place (include/hicmi.h, hicmi_p2_breaks).
    Returns one dict per chromosome: 'score0' (literal objective of the arrangement), 'total', 'table' (the scaffolds'
    (L - 1) x 8 blocks of scores concatenated in arrangement order: row = cut p as laid down, column = candidate
    BREAK_MOVES[k]), 'offsets' (first table row of each scaffold), 'names', 'orientations', 'minPiece' and 'rows' (per
    scaffold in arrangement order: bins, best_cut, cut_after_bin, best_move, best_delta, gain, verdict, and near: how many
    competing candidates lay within NEAR_TOP of the top closed-form score).

    Total, layout and lanes are placementSupport's.  On the device all chromosomes go through one hicmi_p2_breaks_multi
    call, one context each; HICMI_P2_BREAKS_DIRECT=1 scores materialised candidates with hicmi_p2_score instead.
    ``minPiece``: only cuts that leave both pieces at least that many bins compete for the best break."""
    minPiece = max(1, int(minPiece))
    return _table_report(matrix, orderedChromosomes, binList, chromList, "breaks",
                         lambda layout, ids, rev, total: _breaks_direct(layout, ids, rev, total, minPiece),
                         lambda layout, ids, rev, total: (ids, rev, [layout.length[int(i)] for i in ids], total), (minPiece,),
                         lambda *a: _breaks_one(*a, minPiece))


def breakSupportText(results):
    """The report: per chromosome ``### Chromosome grouping i ### score0``, then one tab-separated line per scaffold in
    arrangement order: scaffold, orientation, bins, best_cut, cut_after_bin, best_move, best_delta, gain, verdict.
    Floats are written with repr; a scaffold without a competing candidate (one or two bins, minPiece): NA."""
    text = []
    for k, res in enumerate(results):
        text.append("### Chromosome grouping " + str(k + 1) + " ### " + repr(res["score0"]) + "\n")
        for name, orient, row in zip(res["names"], res["orientations"], res["rows"]):
            text.append("\t".join([name, orient, str(row["bins"])] + [_support_text(row[key]) for key in
                                                                      ("best_cut", "cut_after_bin", "best_move", "best_delta",
                                                                       "gain")] + [row["verdict"]]) + "\n")
    return "".join(text)


def writeBreakSupportToFile(results, outFile, fullDir=None):
    """breakSupportText to ``outFile``; ``fullDir``: also each chromosome's table as ``Chr_i.breaks.tsv``, one line per
    (scaffold, cut) in enumeration order: scaffold, the scaffold's own bins before the cut, the 8 scores."""
    with open(outFile, "w") as fh:
        fh.write(breakSupportText(results))
    if fullDir:
        os.makedirs(fullDir, exist_ok=True)
        for k, res in enumerate(results):
            table = np.asarray(res["table"])
            with open(os.path.join(fullDir, "Chr_%d.breaks.tsv" % (k + 1)), "w") as fh:
                fh.write("\t".join(("scaffold", "cut") + BREAK_MOVES) + "\n")
                for name, orient, row, at in zip(res["names"], res["orientations"], res["rows"], res["offsets"]):
                    L = row["bins"]
                    for p in range(1, L):
                        fh.write("\t".join([name, str(L - p if orient == "-" else p)]
                                           + [repr(float(v)) for v in table[at + p - 1]]) + "\n")
    print("Break support written for scaffolds " + str(sum(len(r["rows"]) for r in results)))


def writeBrokenGroupFile(results, chromosomeGroupFile, outFile):
    """``chromosomeGroupFile`` copied line by line to ``outFile``, except that the lines of every ``breakable`` scaffold
    name it ``NAME.brk1`` for its bins up to the best cut and ``NAME.brk2`` for the rest.  One pass; the input file is
    only read."""
    last = [{name: row["cut_after_bin"] for name, row in zip(res["names"], res["rows"]) if row["verdict"] == "breakable"}
            for res in results]
    if os.path.abspath(outFile) == os.path.abspath(chromosomeGroupFile):
        raise ValueError("the broken group file must not be the chromosomeGroupFile itself")
    chrom = -1
    with open(chromosomeGroupFile) as src, open(outFile, "w") as dst:
        for line in src:
            if line.startswith("#"):
                chrom += 1
            elif 0 <= chrom < len(last) and last[chrom]:
                cols = line.split("\t", 2)
                name = cols[1].rstrip("\r\n") if len(cols) == 2 else cols[1]
                if len(cols) >= 2 and name in last[chrom]:
                    piece = name + (".brk1" if int(cols[0]) <= last[chrom][name] else ".brk2")
                    line = "\t".join([cols[0], piece + cols[1][len(name):]] + cols[2:])
            dst.write(line)
    print("Broken group file written with scaffolds split " + str(sum(len(d) for d in last)))


def breakSupportToFiles(matrix, orderedChromosomes, binList, chromosomeGroupFile, breakSupportFile=None,
                        brokenChromosomeGroupFile=None, fullDir=None, minPiece=1, chromList=None):
    """breakSupport of a resident map and the files wanted of it; returns the results."""
    if chromList is None:
        chromList = _read_groups_quietly(chromosomeGroupFile)
    results = breakSupport(matrix, orderedChromosomes, binList, chromList, minPiece=minPiece)
    if breakSupportFile:
        writeBreakSupportToFile(results, breakSupportFile, fullDir)
    if brokenChromosomeGroupFile:
        writeBrokenGroupFile(results, chromosomeGroupFile, brokenChromosomeGroupFile)
    return results


# ---- inversion support of a finished ordering ------------------------------------------
def inversion_counts(S, maxSpan=0):
    """(S, S) mask of the candidates that compete for a left end's best inversion: row i, column j = scaffolds i ... j
    reversed and flipped, with j > i (j = i is placement support's in-place flip), not (0, S - 1) (the chromosome read
    backwards: the same objective) and, with ``maxSpan`` > 0, at most maxSpan scaffolds (include/hicmi.h,
    hicmi_p2_inversions)."""
    i, j = np.indices((S, S))
    m = j > i
    if S > 1:
        m[0, S - 1] = False
    if maxSpan > 0:
        m &= j - i + 1 <= maxSpan
    return m


def inversion_work(lengths, maxSpan=0):
    """Matrix elements that one chromosome's table reads: the sum of len * (n - len) over the computed candidates
    (i <= j, at most ``maxSpan`` scaffolds when > 0), len the bins of the segment - the figure hicmi_p2_inversions_multi
    holds against its bound of 1e13 per call."""
    pos = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    n, S, work = int(pos[-1]), len(lengths), 0
    for i in range(S):
        seg = pos[i + 1:(i + maxSpan if maxSpan > 0 else S) + 1] - pos[i]
        work += int(np.sum(seg * (n - seg)))
    return work


def inversion_summary(table, maxSpan=0):
    """What hicmi_p2_inversions returns as ``best`` from an S x S table of scores: per left end [j of the first maximum
    over inversion_counts, or -1; how many competing candidates lie within NEAR_TOP of it]."""
    flat = np.asarray(table, dtype=np.float64)
    S = len(flat)
    counts = inversion_counts(S, maxSpan)
    out = np.zeros((S, 2), np.int32)
    for i in range(S):
        ok = counts[i] & np.isfinite(flat[i])
        if not ok.any():
            out[i] = (-1, 0)
            continue
        v = np.where(ok, flat[i], -np.inf)
        top = float(v.max())
        out[i] = (int(np.argmax(v)), int(np.count_nonzero(v >= top - abs(top) * NEAR_TOP)))
    return out


def _inversion_row(layout, ids, rev, i, j):
    """Bin order (selection indices) of "the arrangement with its scaffolds i ... j in reverse order, each flipped"."""
    oi = [int(v) for v in ids]
    orr = [int(v) for v in rev]
    oi[i:j + 1] = oi[i:j + 1][::-1]
    orr[i:j + 1] = [1 - r for r in orr[i:j + 1][::-1]]
    return layout.node_row(oi, orr)


def _inversions_direct(layout, ids, rev, total, maxSpan):
    """A/B path (HICMI_P2_INVERT_DIRECT=1): the same table from hicmi_p2_score on every computed candidate's materialised
    bin order, at most SUPPORT_DIRECT_BYTES of rows at a time."""
    S = len(ids)
    table = np.zeros((S, S))
    if layout.n < 2 or not total > 0:
        return table, np.tile(np.array([-1, 0], np.int32), (S, 1))
    cands = [(i, j) for i in range(S) for j in range(i, S) if maxSpan <= 0 or j - i + 1 <= maxSpan]
    flat = np.zeros(len(cands))
    _score_rows(layout, total, flat, lambda c: _inversion_row(layout, ids, rev, *cands[c]))
    for (i, j), v in zip(cands, flat):
        table[i, j] = v
    return table, inversion_summary(table, maxSpan)


def _inversions_one(layout, ids, rev, total, table, best, group, maxSpan):
    """One chromosome's result from its table: score0, the best inversion of every left end and the verdicts (the picks:
    _decide_near).  The reported floats are literal scores - the arrangement and every best inversion of the chromosome
    in one call - so that they do not depend on how the table was computed."""
    S = len(ids)
    lengths = [layout.length[int(i)] for i in ids]
    live = layout.n >= 2 and total > 0
    counts = inversion_counts(S, maxSpan)
    nears = [int(best[i][1]) if live else 0 for i in range(S)]
    picks = [int(best[i][0]) if live else -1 for i in range(S)]
    for i in range(S):
        if picks[i] >= 0 and nears[i] > 1:
            picks[i] = _decide_near(table[i], counts[i], picks[i], lambda c: _inversion_row(layout, ids, rev, i, c), layout,
                                    total)
    moves = [i for i in range(S) if picks[i] >= 0]
    lit = _literal_rows(layout, [layout.node_row(ids, rev)] + [_inversion_row(layout, ids, rev, i, picks[i]) for i in moves],
                        total) if live else [0.0]
    score0 = float(lit[0])
    delta_of = dict(zip(moves, (float(v) - score0 for v in lit[1:])))
    rows = []
    for i in range(S):
        delta = delta_of.get(i)
        if delta is None:
            end = end_name = span = span_bins = gain = None
            verdict = "NA"
        else:
            end = picks[i]
            end_name, span, span_bins = group[end].name, end - i + 1, sum(lengths[i:end + 1])
            gain = delta / score0
            verdict = "invertible" if delta > 0 else "supported"
        rows.append({"bins": lengths[i], "best_j": end, "best_end": end_name, "span": span, "span_bins": span_bins,
                     "best_delta": delta, "gain": gain, "verdict": verdict, "near": nears[i]})
    return {"score0": score0, "total": total, "table": table, "rows": rows, "maxSpan": maxSpan}


def inversionSupport(matrix: GenomeMatrix, orderedChromosomes, binList, chromList=None, maxSpan=0):
    """Which runs of consecutive scaffolds the map would rather read backwards: for every pair i <= j of every
    chromosome, the scaffolds i ... j in reverse order, each flipped (include/hicmi.h,
    hicmi_p2_inversions).  Returns one dict per chromosome: 'score0' (literal objective of the arrangement), 'total',
    'table' (S x S scores: row = first scaffold of the segment, column = last; 0.0 below the diagonal and beyond
    ``maxSpan`` scaffolds), 'names', 'orientations', 'maxSpan' and 'rows' (per scaffold in arrangement order, as the left
    end of a segment: bins, best_j, best_end, span, span_bins, best_delta, gain, verdict, and near: how many competing
    candidates lay within NEAR_TOP of the top closed-form score).

    Total, layout and lanes are placementSupport's.  On the device all chromosomes go through one
    hicmi_p2_inversions_multi call, one context each; HICMI_P2_INVERT_DIRECT=1 scores materialised candidates with
    hicmi_p2_score instead.  ``maxSpan`` > 0: only segments of at most that many scaffolds are computed and compete."""
    maxSpan = max(0, int(maxSpan))
    return _table_report(matrix, orderedChromosomes, binList, chromList, "inversions",
                         lambda layout, ids, rev, total: _inversions_direct(layout, ids, rev, total, maxSpan),
                         lambda layout, ids, rev, total: (ids, rev, total), (maxSpan,),
                         lambda *a: _inversions_one(*a, maxSpan), switch="HICMI_P2_INVERT_DIRECT")


def inversionSupportText(results):
    """The report: per chromosome ``### Chromosome grouping i ### score0``, then one tab-separated line per scaffold in
    arrangement order, as the left end of a segment: scaffold, orientation, bins, best_end, span, span_bins, best_delta,
    gain, verdict.  Floats are written with repr; a left end without a competing candidate: NA."""
    text = []
    for k, res in enumerate(results):
        text.append("### Chromosome grouping " + str(k + 1) + " ### " + repr(res["score0"]) + "\n")
        for name, orient, row in zip(res["names"], res["orientations"], res["rows"]):
            text.append("\t".join([name, orient, str(row["bins"])] + [_support_text(row[key]) for key in
                                                                      ("best_end", "span", "span_bins", "best_delta", "gain")]
                                  + [row["verdict"]]) + "\n")
    return "".join(text)


def writeInversionSupportToFile(results, outFile, fullDir=None):
    """inversionSupportText to ``outFile``; ``fullDir``: also each chromosome's S x S table as ``Chr_i.inversions.tsv``
    (row = first scaffold of the segment, columns = last scaffold)."""
    with open(outFile, "w") as fh:
        fh.write(inversionSupportText(results))
    if fullDir:
        os.makedirs(fullDir, exist_ok=True)
        for k, res in enumerate(results):
            with open(os.path.join(fullDir, "Chr_%d.inversions.tsv" % (k + 1)), "w") as fh:
                fh.write("\t".join(["scaffold"] + list(res["names"])) + "\n")
                for name, line in zip(res["names"], np.asarray(res["table"])):
                    fh.write("\t".join([name] + [repr(float(v)) for v in line]) + "\n")
    print("Inversion support written for scaffolds " + str(sum(len(r["rows"]) for r in results)))


# ---- refinement: the best relocation or inversion applied, round by round ---------------
REFINE_MOVES = ("relocate", "invert")


def choose_move(rel_rows, inv_rows, score0, minGain=0.0):
    """The move of one round for one chromosome, or None when it has converged.  ``rel_rows[j]``: (gap, reversed,
    literal delta) of scaffold j's decided best relocation or None; ``inv_rows[i]``: (j, literal delta) of left end i's
    decided best inversion or None.  The first strict maximum of the deltas wins, relocations j = 0 ... S-1 before
    inversions i = 0 ... S-2; it is applied only if its delta is > 0 and > minGain * |score0|.  Returns
    ("relocate", j, gap, reversed, delta) or ("invert", i, j, delta)."""
    best, top = None, -math.inf
    for j, row in enumerate(rel_rows or ()):
        if row is not None and row[2] > top:
            best, top = ("relocate", j, int(row[0]), int(row[1]), float(row[2])), float(row[2])
    for i, row in enumerate(inv_rows or ()):
        if row is not None and row[1] > top:
            best, top = ("invert", i, int(row[0]), float(row[1])), float(row[1])
    if best is None or not top > 0 or not top > minGain * abs(score0):
        return None
    return best


def apply_move(ids, rev, move):
    """(ids, rev) as lists after ``move`` (choose_move): a relocation takes scaffold j out and puts it back at gap g of
    the arrangement without it in the given orientation; an inversion reverses the scaffolds i ... j and flips each."""
    ids, rev = [int(v) for v in ids], [int(v) for v in rev]
    if move[0] == "relocate":
        _kind, j, gap, r, _delta = move
        sid = ids.pop(j)
        rev.pop(j)
        ids.insert(gap, sid)
        rev.insert(gap, int(r))
    elif move[0] == "invert":
        _kind, i, j, _delta = move
        ids[i:j + 1] = ids[i:j + 1][::-1]
        rev[i:j + 1] = [1 - r for r in rev[i:j + 1][::-1]]
    else:
        raise ValueError("unknown move " + repr(move[0]))
    return ids, rev


def _moved_group(group, move):
    """A chromosome's Scaffold list after ``move``: copies, flipped where the move flips them."""
    order, flip = apply_move(range(len(group)), [0] * len(group), move)
    if move[0] == "relocate":                                 # apply_move sets the orientation; a flip is a change of it
        flip = [int(k == move[1] and (group[k].orientation == "-") != bool(move[3])) for k in order]
    out = []
    for k, f in zip(order, flip):
        s = group[k].copy()
        if f:
            s.flipOrientation()
        out.append(s)
    return out


def refineOrdering(matrix: GenomeMatrix, orderedChromosomes, binList, chromList, moves=REFINE_MOVES, maxSpan=0, minGain=0.0,
                   maxRounds=100):
    """Hill climbing from a finished ordering.  One round, for every chromosome that has not converged:
    the placement table (placementSupport) and the inversion table (inversionSupport), one multi call each for all of
    them; each scaffold's decided best relocation and each left end's decided best inversion with their literal
    deltas; the move of the round (choose_move) applied, or the chromosome has converged.  One move per chromosome per
    round, because the tables are stale after a move; every accepted move strictly raises a literal score, so the loop
    ends, and ``maxRounds`` caps it.  ``moves``: the families tried.  Returns (the refined ordering, the log: one dict
    per applied move - round, chromosome, kind, scaffold, to, from / to as text, before, after -, the summary: one
    dict per chromosome - before, after, moves, rounds, converged)."""
    moves = tuple(moves)
    if not moves or any(m not in REFINE_MOVES for m in moves):
        raise ValueError("moves must be taken from " + ",".join(REFINE_MOVES))
    current = [list(group) for group in orderedChromosomes]
    summary = [{"before": None, "after": None, "moves": 0, "rounds": 0, "converged": False} for _g in current]
    log = []
    for rnd in range(1, int(maxRounds) + 1):
        todo = [k for k, s in enumerate(summary) if not s["converged"]]
        if not todo:
            break
        sub = [current[k] for k in todo]
        sub_list = None if chromList is None else [chromList[k] for k in todo]
        rel = placementSupport(matrix, sub, binList, sub_list) if "relocate" in moves else None
        inv = inversionSupport(matrix, sub, binList, sub_list, maxSpan=maxSpan) if "invert" in moves else None
        for at, k in enumerate(todo):
            res = rel[at] if rel is not None else inv[at]
            score0 = res["score0"]
            rel_rows = inv_rows = None
            if rel is not None:
                rel_rows = [None if r["best_delta"] is None else (r["best_gap"], r["best_orientation"] == "-", r["best_delta"])
                            for r in rel[at]["rows"]]
            if inv is not None:
                inv_rows = [None if r["best_delta"] is None else (r["best_j"], r["best_delta"]) for r in inv[at]["rows"]]
            stat = summary[k]
            if stat["before"] is None:
                stat["before"] = score0
            stat["after"], stat["rounds"] = score0, rnd
            move = choose_move(rel_rows, inv_rows, score0, minGain)
            if move is None:
                stat["converged"] = True
                continue
            group = current[k]
            if move[0] == "relocate":
                what, src, dst = group[move[1]].name, "%d%s" % (move[1], group[move[1]].orientation), \
                    "%d%s" % (move[2], "-" if move[3] else "+")
            else:
                what, src, dst = group[move[1]].name + ".." + group[move[2]].name, "%d..%d" % (move[1], move[2]), "reversed"
            current[k] = _moved_group(group, move)
            stat["moves"] += 1
            stat["after"] = score0 + move[-1]
            log.append({"round": rnd, "chromosome": k + 1, "kind": move[0], "scaffold": what, "from": src, "to": dst,
                        "before": score0, "after": score0 + move[-1], "move": move})
    return current, log, summary


def writeRefinement(refined, log, summary, outDir, chromosomeOrderFile, plotOrderFile):
    """The refined ordering through the existing writers as ``outDir``/basename of the two files, ``refine.log`` (one
    line per applied move: round, chromosome, kind, scaffold(s), from -> to, score before, score after) and
    ``refine_summary.tsv`` (per chromosome: score before and after, moves, rounds, converged)."""
    os.makedirs(outDir, exist_ok=True)
    order_out = os.path.join(outDir, os.path.basename(chromosomeOrderFile))
    writeScaffoldOrderingsToFile(refined, order_out)
    writeBinIDsOrderingToFile([s for group in refined for s in group], os.path.join(outDir, os.path.basename(plotOrderFile)))
    with open(os.path.join(outDir, "refine.log"), "w") as fh:
        for e in log:
            fh.write("\t".join([str(e["round"]), str(e["chromosome"]), e["kind"], e["scaffold"], e["from"] + " -> " + e["to"],
                                repr(e["before"]), repr(e["after"])]) + "\n")
    with open(os.path.join(outDir, "refine_summary.tsv"), "w") as fh:
        fh.write("chromosome\tscore_before\tscore_after\tmoves\trounds\tconverged\n")
        for k, s in enumerate(summary):
            fh.write("\t".join([str(k + 1), repr(s["before"]), repr(s["after"]), str(s["moves"]), str(s["rounds"]),
                                "yes" if s["converged"] else "no"]) + "\n")
    print("Refinement moves applied " + str(len(log)))
    return order_out


# ---- junction support of a finished ordering --------------------------------------------
JUNCTION_WINDOW = 16       # bins of a side (0: the whole block)
JUNCTION_MIN_REL = 0.25    # J / ref at or above which a junction holds


def junction_records(lengths, boundaries, window=JUNCTION_WINDOW):
    """The records of a junction-support call (include/hicmi.h, hicmi_junction_sums) for chromosomes of ``lengths[c]``
    bins laid one after the other, chromosome c at offset sum(lengths[:c]).  ``boundaries[c]``: the positions inside
    chromosome c at which a scaffold other than its first begins, strictly ascending in 1 .. lengths[c] - 1.  A side is
    cut to its first ``window`` bins (0: the whole block) and never leaves its chromosome.  Returns a dict: 'rec' (int64,
    n_rec x 6: startA, stepA, lenA, startB, stepB, lenB), first the internal junctions - 'internal': (chromosome,
    boundary index) each, A the bins to the left read leftwards, B those to the right read rightwards - then the end
    pairs - 'pairs': (e, f) with e < f on different chromosomes, end 2 c the head of chromosome c (read from its first bin
    inwards) and 2 c + 1 its tail (from its last bin inwards) - and 'G', 'lengths', 'window'."""
    window = int(window)
    if window < 0:
        raise ValueError("window must be 0 (the whole block) or a positive number of bins")
    lengths = [int(v) for v in lengths]
    if any(v < 1 for v in lengths):
        raise ValueError("every chromosome needs at least one bin")
    cut = (lambda v: min(v, window)) if window else (lambda v: v)
    rec, internal, off = [], [], 0
    offsets = []
    for c, (n, bounds) in enumerate(zip(lengths, boundaries)):
        offsets.append(off)
        last = 0
        for k, p in enumerate(bounds):
            p = int(p)
            if not last < p < n:
                raise ValueError("chromosome %d: scaffold boundaries must ascend strictly inside 1 .. %d" % (c + 1, n - 1))
            rec.append((off + p - 1, -1, cut(p), off + p, 1, cut(n - p)))
            internal.append((c, k))
            last = p
        off += n
    G = len(lengths)
    side = []
    for c in range(G):
        side.append((offsets[c], 1, cut(lengths[c])))                       # head
        side.append((offsets[c] + lengths[c] - 1, -1, cut(lengths[c])))     # tail
    pairs = [(e, f) for e in range(2 * G) for f in range(e + 1, 2 * G) if e // 2 != f // 2]
    rec.extend(side[e] + side[f] for e, f in pairs)
    return {"rec": np.array(rec, dtype=np.int64).reshape(len(rec), 6), "internal": internal, "pairs": pairs, "G": G,
            "lengths": lengths, "window": window}


def junction_norm(lenA, lenB):
    """sum over d = 1 .. lenA + lenB - 1 of cnt(d) * (1.0 / d), d ascending: cnt(d) pairs (a, b) have a + b + 1 = d."""
    lenA, lenB = int(lenA), int(lenB)
    d = np.arange(1, lenA + lenB, dtype=np.float64)
    cnt = np.minimum(np.minimum(d, lenA + lenB - d), float(min(lenA, lenB)))
    return float(np.cumsum(cnt * (1.0 / d))[-1])              # cumsum adds left to right: the loop's bits


def junction_summary(sums, records, minRel=JUNCTION_MIN_REL):
    """Every decision of the junction report from the downloaded ``sums`` of junction_records' ``records`` (DESIGN.md
    9k).  J = sum / junction_norm; 'ref': numpy.median of J over the internal junctions, None without one or when it is
    0.  'internal': per internal junction chromosome, boundary, bins_left, bins_right, J, rel, verdict (held: rel >=
    minRel, else weak).  'table': the 2G x 2G J of the ends, exactly symmetric, NaN inside one chromosome.  'ends': per
    end best (the first maximum of its row), J, rel, mutual (each is the other's best), second (the best end of a
    chromosome other than best's; None when G = 2), second_J, verdict (joinable: mutual and rel >= minRel, else free).
    rel and the verdicts are None without ref, an end's every field when G = 1.  'joinable': (e, f, J) with e < f;
    'weak': (chromosome, boundary)."""
    rec, G = records["rec"], records["G"]
    norms = {}

    def J_of(r):
        key = (int(rec[r][2]), int(rec[r][5]))
        if key not in norms:
            norms[key] = junction_norm(*key)
        return float(sums[r]) / norms[key]
    n_int = len(records["internal"])
    J_int = [J_of(r) for r in range(n_int)]
    ref = float(np.median(J_int)) if n_int else None
    if ref is not None and not ref > 0:
        ref = None
    internal, weak = [], []
    for r, (c, k) in enumerate(records["internal"]):
        rel = J_int[r] / ref if ref is not None else None
        verdict = None if rel is None else ("held" if rel >= minRel else "weak")
        if verdict == "weak":
            weak.append((c, k))
        internal.append({"chromosome": c, "boundary": k, "bins_left": int(rec[r][2]), "bins_right": int(rec[r][5]),
                         "J": J_int[r], "rel": rel, "verdict": verdict})
    table = np.full((2 * G, 2 * G), np.nan)
    for r, (e, f) in enumerate(records["pairs"], start=n_int):
        table[e, f] = table[f, e] = J_of(r)

    def first_max(e, skip):
        at, top = None, -math.inf
        for f in range(2 * G):
            if f // 2 not in skip and table[e, f] > top:
                at, top = f, float(table[e, f])
        return at
    best = [first_max(e, (e // 2,)) for e in range(2 * G)] if G > 1 else [None] * (2 * G)
    window = records["window"]
    ends, joinable = [], []
    for e in range(2 * G):
        f, bins = best[e], min(records["lengths"][e // 2], window) if window else records["lengths"][e // 2]
        if f is None:
            ends.append({"bins": bins, "best": None, "J": None, "rel": None, "mutual": None, "second": None,
                         "second_J": None, "verdict": None})
            continue
        J = float(table[e, f])
        rel = J / ref if ref is not None else None
        mutual = best[f] == e
        second = first_max(e, (e // 2, f // 2)) if G > 2 else None
        verdict = None if rel is None else ("joinable" if mutual and rel >= minRel else "free")
        if verdict == "joinable" and e < f:
            joinable.append((e, f, J))
        ends.append({"bins": bins, "best": f, "J": J, "rel": rel, "mutual": mutual, "second": second,
                     "second_J": None if second is None else float(table[e, second]), "verdict": verdict})
    return {"ref": ref, "window": window, "minRel": float(minRel), "internal": internal, "table": table,
            "ends": ends, "joinable": joinable, "weak": weak}


def _flipped(item):
    return (item[0], "-" if item[1] == "+" else "+")


def join_chromosomes(ordered, joins):
    """``ordered``: per chromosome its (scaffold, '+'/'-') pairs in order; ``joins``: (e, f, J) joins of chromosome ends
    (end 2 c: the head of chromosome c, 2 c + 1: its tail), every end in at most one of them, so the chromosomes form
    paths and cycles.  A cycle drops its smallest-J join, the first listed on a tie.  A joined chromosome is read in the
    direction that keeps its lowest-numbered member as written; a member entered through its tail is reversed: scaffold
    order reversed, every orientation flipped.  It stands at the position of its lowest-numbered member and all other
    chromosomes keep their order.  Returns (the new chromosomes, per new chromosome its members as (old chromosome,
    reversed), the joins applied, the joins dropped)."""
    G = len(ordered)
    joins = [(int(e), int(f), float(J)) for e, f, J in joins]
    partner = {}
    for at, (e, f, _J) in enumerate(joins):
        if e // 2 == f // 2 or e in partner or f in partner or not (0 <= e < 2 * G and 0 <= f < 2 * G):
            raise ValueError("joins must pair each end at most once, across chromosomes")
        partner[e], partner[f] = (f, at), (e, at)
    dropped, seen = set(), set()
    for c in range(G):                                        # cycles: walk from c's tail until an open end or c again
        if c in seen:
            continue
        cur, used, path = 2 * c + 1, [], [c]
        while cur in partner:
            nxt, at = partner[cur]
            used.append(at)
            if nxt // 2 == c:                                 # back at the start: a cycle
                worst = min(used, key=lambda a: (joins[a][2], a))
                dropped.add(worst)
                break
            path.append(nxt // 2)
            cur = nxt ^ 1
        seen.update(path)
    live = {e: f for e, (f, at) in partner.items() if at not in dropped}
    out, members, placed = [], [], set()
    for c in range(G):
        if c in placed:
            continue
        cur, end = c, 2 * c                                   # c is the lowest-numbered member of its path: leftwards
                                                              # from its head to the start of the path
        while end in live:
            end = live[end] ^ 1
            cur = end // 2
        chrom, mem = [], []
        while True:                                           # `end`: the end the member is entered through
            rev = bool(end & 1)
            group = ordered[cur]
            chrom.extend([_flipped(s) for s in group[::-1]] if rev else list(group))
            mem.append((cur, rev))
            if end ^ 1 not in live:
                break
            end = live[end ^ 1]
            cur = end // 2
        placed.update(k for k, _rev in mem)
        out.append(chrom)
        members.append(mem)
    applied = [j for at, j in enumerate(joins) if at not in dropped]
    return out, members, applied, [joins[at] for at in sorted(dropped)]


def cut_chromosomes(ordered, weak):
    """``ordered`` as for join_chromosomes with every chromosome split at its ``weak`` junctions, (chromosome, boundary k:
    between its scaffolds k and k + 1); the pieces stand where the chromosome stood.  Returns (the new chromosomes, per
    new chromosome (old chromosome, first scaffold, one past its last))."""
    cuts = {}
    for c, k in weak:
        if not (0 <= c < len(ordered) and 0 <= k < len(ordered[c]) - 1):
            raise ValueError("no junction %d in chromosome %d" % (k, c + 1))
        cuts.setdefault(int(c), set()).add(int(k) + 1)
    out, members = [], []
    for c, group in enumerate(ordered):
        edges = [0] + sorted(cuts.get(c, ())) + [len(group)]
        for a, b in zip(edges[:-1], edges[1:]):
            out.append(list(group[a:b]))
            members.append((c, a, b))
    return out, members


def junctionSupport(matrix: GenomeMatrix, orderedChromosomes, binList, chromList=None, window=JUNCTION_WINDOW,
                    minRel=JUNCTION_MIN_REL):
    """Which chromosome ends belong together and which scaffold junctions do not hold (include/hicmi.h,
    hicmi_junction_sums): the mean contact, weighted 1 / distance, across every scaffold boundary of every ordered
    chromosome and between every two ends of different chromosomes, on the genome context's matrix as it stands, in ONE
    native call.  Returns junction_summary's dict with 'chromosomes' added: per chromosome its names, orientations and
    scaffold bin counts.  ``chromList`` is accepted for the signature the reports share; the bins come from the ordered
    scaffolds themselves."""
    where = matrix.bin_index(binList)
    bins, lengths, boundaries = [], [], []
    for group in orderedChromosomes:
        at, bounds = 0, []
        for s in group:
            if at:
                bounds.append(at)
            at += len(s.binList)
            bins.extend(where[b] for b in s.binList)
        lengths.append(at)
        boundaries.append(bounds)
    records = junction_records(lengths, boundaries, window)
    sums = matrix.ctx.junction_sums(np.asarray(bins, dtype=np.int32), records["rec"]) if len(records["rec"]) \
        else np.zeros(0)
    res = junction_summary(sums, records, minRel)
    res["sums"], res["rec"] = np.asarray(sums), records["rec"]
    res["chromosomes"] = [{"names": [s.name for s in group], "orientations": [s.orientation for s in group],
                           "bins": [len(s.binList) for s in group]} for group in orderedChromosomes]
    return res


_END_NAME = ("head", "tail")


def junctionSupportText(results):
    """The report: ``### reference ref window W minRel r``; per chromosome ``### Chromosome grouping i ###`` and one
    tab-separated line per internal junction: left scaffold, right scaffold, bins_left, bins_right, J, rel, verdict; then
    ``### Chromosome ends ###`` and one line per end: chromosome, head/tail, the terminal scaffold, bins,
    best_chromosome, best_end, J, rel, mutual, second_chromosome, second_J, verdict.  Floats are written with repr,
    what does not exist as NA."""
    text = ["### reference %s window %d minRel %s\n" % (_support_text(results["ref"]), results["window"],
                                                        repr(results["minRel"]))]
    rows = iter(results["internal"])
    for k, chrom in enumerate(results["chromosomes"]):
        text.append("### Chromosome grouping " + str(k + 1) + " ###\n")
        for left, right in zip(chrom["names"][:-1], chrom["names"][1:]):
            row = next(rows)
            text.append("\t".join([left, right, str(row["bins_left"]), str(row["bins_right"]), repr(row["J"]),
                                   _support_text(row["rel"]), row["verdict"] or "NA"]) + "\n")
    text.append("### Chromosome ends ###\n")
    for e, row in enumerate(results["ends"]):
        chrom = results["chromosomes"][e // 2]
        f, g = row["best"], row["second"]
        text.append("\t".join([str(e // 2 + 1), _END_NAME[e & 1], chrom["names"][-1 if e & 1 else 0], str(row["bins"]),
                               "NA" if f is None else str(f // 2 + 1), "NA" if f is None else _END_NAME[f & 1],
                               _support_text(row["J"]), _support_text(row["rel"]),
                               "NA" if row["mutual"] is None else ("yes" if row["mutual"] else "no"),
                               "NA" if g is None else str(g // 2 + 1), _support_text(row["second_J"]),
                               row["verdict"] or "NA"]) + "\n")
    return "".join(text)


def writeJunctionSupportToFile(results, outFile, fullDir=None):
    """junctionSupportText to ``outFile``; ``fullDir``: also the 2G x 2G table of J between the ends as
    ``junctions.ends.tsv`` (rows and columns 1.head, 1.tail, 2.head, ...; NA inside one chromosome)."""
    with open(outFile, "w") as fh:
        fh.write(junctionSupportText(results))
    if fullDir:
        os.makedirs(fullDir, exist_ok=True)
        labels = ["%d.%s" % (e // 2 + 1, _END_NAME[e & 1]) for e in range(len(results["ends"]))]
        with open(os.path.join(fullDir, "junctions.ends.tsv"), "w") as fh:
            fh.write("\t".join(["end"] + labels) + "\n")
            for label, line in zip(labels, results["table"]):
                fh.write("\t".join([label] + ["NA" if v != v else repr(float(v)) for v in line]) + "\n")
    print("Junction support written for junctions " + str(len(results["internal"])) + " and chromosome ends "
          + str(len(results["ends"])))


def _group_file_lines(chromosomeGroupFile):
    """Per group of ``chromosomeGroupFile`` its lines verbatim without the header (the first line is group 1's header:
    readChromsFromFile), each ending in a newline."""
    with open(chromosomeGroupFile) as fh:
        lines = fh.read().splitlines(keepends=True)
    groups = []
    for k, line in enumerate(lines):
        if k == 0 or line[0] == "#":
            groups.append([])
        else:
            groups[-1].append(line if line.endswith("\n") else line + "\n")
    return groups


def _write_regrouped(new_groups, new_lines, outDir, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile):
    """The three files of a regrouped ordering as ``outDir``/basename of the input files: the group file with one
    ``### Chromosome group i ###`` header per new chromosome over ``new_lines[i]``, the order file and the plot-order file
    through the existing writers.  The input files are only read."""
    os.makedirs(outDir, exist_ok=True)
    names = [os.path.join(outDir, os.path.basename(f)) for f in (chromosomeGroupFile, chromosomeOrderFile, plotOrderFile)]
    if len(set(names)) != 3:
        raise ValueError("the group, order and plot-order files need three different names")
    for new, old in zip(names, (chromosomeGroupFile, chromosomeOrderFile, plotOrderFile)):
        if os.path.abspath(new) == os.path.abspath(old):
            raise ValueError("the regrouped files must not replace the input files: " + old)
    with open(names[0], "w") as fh:
        for k, lines in enumerate(new_lines):
            fh.write("### Chromosome group " + str(k + 1) + " ###\n" + "".join(lines))
    writeScaffoldOrderingsToFile(new_groups, names[1])
    writeBinIDsOrderingToFile([s for group in new_groups for s in group], names[2])
    return names


def _plain(orderedChromosomes):
    return [[(s.name, s.orientation) for s in group] for group in orderedChromosomes]


def writeJoinedFiles(results, orderedChromosomes, outDir, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile):
    """The ordering with every ``joinable`` pair of chromosome ends joined (join_chromosomes), as a group file, an order
    file and a plot-order file in ``outDir`` under the input files' names, and ``joins.log``: one line per join -
    ``joined`` or ``dropped`` (the smallest join of a cycle), chromosome, end, chromosome, end, J, rel.  A joined group
    holds its members' lines of the group file verbatim, lowest-numbered member first.  Returns the new chromosomes."""
    _plainly, members, applied, dropped = join_chromosomes(_plain(orderedChromosomes), results["joinable"])
    old_lines = _group_file_lines(chromosomeGroupFile)
    new_groups, new_lines = [], []
    for mem in members:
        group = []
        for c, rev in mem:
            if rev:
                for s in orderedChromosomes[c][::-1]:
                    s = s.copy()
                    s.flipOrientation()
                    group.append(s)
            else:
                group.extend(orderedChromosomes[c])
        new_groups.append(group)
        new_lines.append([line for c in sorted(c for c, _r in mem) for line in old_lines[c]])
    _write_regrouped(new_groups, new_lines, outDir, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile)
    ref = results["ref"]
    with open(os.path.join(outDir, "joins.log"), "w") as fh:
        for what, joins in (("joined", applied), ("dropped", dropped)):
            for e, f, J in joins:
                fh.write("\t".join([what, str(e // 2 + 1), _END_NAME[e & 1], str(f // 2 + 1), _END_NAME[f & 1], repr(J),
                                    _support_text(None if ref is None else J / ref)]) + "\n")
    print("Chromosome ends joined " + str(len(applied)))
    return new_groups


def writeCutFiles(results, orderedChromosomes, outDir, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile):
    """The ordering with every chromosome split at its ``weak`` junctions (cut_chromosomes), as the same three files in
    ``outDir``, and ``cuts.log``: one line per cut - chromosome, left scaffold, right scaffold, J, rel.  A piece holds the
    group file's lines of its scaffolds verbatim, in the file's order.  Returns the new chromosomes."""
    _plainly, members = cut_chromosomes(_plain(orderedChromosomes), results["weak"])
    old_lines = _group_file_lines(chromosomeGroupFile)
    new_groups, new_lines = [], []
    for c, a, b in members:
        group = orderedChromosomes[c][a:b]
        mine = {s.name for s in group}
        new_groups.append(group)
        new_lines.append([line for line in old_lines[c] if line.rstrip("\r\n").split("\t", 2)[1] in mine])
    _write_regrouped(new_groups, new_lines, outDir, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile)
    weak = set(results["weak"])
    with open(os.path.join(outDir, "cuts.log"), "w") as fh:
        for row in results["internal"]:
            if (row["chromosome"], row["boundary"]) in weak:
                names = results["chromosomes"][row["chromosome"]]["names"]
                fh.write("\t".join([str(row["chromosome"] + 1), names[row["boundary"]], names[row["boundary"] + 1],
                                    repr(row["J"]), _support_text(row["rel"])]) + "\n")
    print("Chromosomes cut at weak junctions " + str(len(weak)))
    return new_groups


def junctionSupportToFiles(matrix, orderedChromosomes, binList, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile,
                           junctionSupportFile=None, joinedDir=None, cutDir=None, fullDir=None, window=JUNCTION_WINDOW,
                           minRel=JUNCTION_MIN_REL):
    """junctionSupport of a resident map and the files wanted of it; returns the results.  Joins and cuts are never
    applied in one file: ``joinedDir`` and ``cutDir`` must differ."""
    if joinedDir and cutDir and os.path.abspath(joinedDir) == os.path.abspath(cutDir):
        raise ValueError("the joined files and the cut files need directories of their own")
    results = junctionSupport(matrix, orderedChromosomes, binList, window=window, minRel=minRel)
    if junctionSupportFile:
        writeJunctionSupportToFile(results, junctionSupportFile, fullDir)
    if joinedDir:
        writeJoinedFiles(results, orderedChromosomes, joinedDir, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile)
    if cutDir:
        writeCutFiles(results, orderedChromosomes, cutDir, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile)
    return results


def getChromosomeOutlineCoords(orderedChromosomes):
    """OG:662-674."""
    coords, index = [], 0
    for group in orderedChromosomes:
        index += sum(len(s.binList) for s in group)
        coords.append(index)
    return coords


def _read_groups_quietly(chromosomeGroupFile):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return readChromsFromFile(chromosomeGroupFile)


def runPipeline(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile,
                savePlotsDirectory, chromosomePlotSuffix, fullGenomePlot, fullGenomePlotTitle, plotOrderFile,
                nScaffolds, scanScaffolds, resolution, device=0, resident=None, placementSupportFile=None,
                breakSupportFile=None, brokenChromosomeGroupFile=None, inversionSupportFile=None,
                refinedChromosomeOrderFile=None, junctionSupportFile=None, joinedFilesDirectory=None):
    """OG:679-712, same positional arguments (``device``, ``resident`` and the ``...File`` keywords are optional extras).

    ``placementSupportFile``: also write the placement-support report of the final ordering there (placementSupport).
    ``breakSupportFile`` / ``brokenChromosomeGroupFile``: also write the break-support report and the group file with
    the breakable scaffolds split (breakSupport).
    ``inversionSupportFile``: also write the inversion-support report there (inversionSupport).
    ``refinedChromosomeOrderFile``: also write the ordering after refineOrdering's hill climb there, as an order file.
    ``junctionSupportFile`` / ``joinedFilesDirectory``: also write the junction-support report there, and the group,
    order and plot-order files with the joinable chromosome ends joined into that directory (junctionSupport).

    ``resident=(DeviceMatrix, bins of its rows)`` from Part 1's ``runPipeline(..., keep_resident=True)``: the contact
    matrix already in HBM is used instead of parsing the HiC-Pro text again.  The reference re-loads the matrix
    restricted to the grouped bins (OG:688-690); here the grouped bins are selected by ID from the full resident
    matrix (raw contacts, .bed order) - the same cells, and bins outside every group are never touched."""
    print("########################################")
    print("### Working on Part2 of the pipeline ###")
    t0 = time.time()
    if resident is not None:
        adjMat, binList = GenomeMatrix(resident[0].ctx), resident[1]
    else:
        binDict = readGroupingsToValidBins(chromosomeGroupFile)
        binList = initiateLoci(hicProBedFile, hicProBiasFile, binID_dict=binDict)
        adjMat = buildAdjacencyMatrix(hicProMatrixFile, binList, device=device)
    try:
        orderedChromosomes = runResident(adjMat, binList, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile,
                                         nScaffolds, scanScaffolds, resolution, savePlotDir=savePlotsDirectory,
                                         plotTitleSuffix=chromosomePlotSuffix)
        if placementSupportFile:
            writePlacementSupportToFile(placementSupport(adjMat, orderedChromosomes, binList,
                                                         _read_groups_quietly(chromosomeGroupFile)), placementSupportFile)
        if breakSupportFile or brokenChromosomeGroupFile:
            breakSupportToFiles(adjMat, orderedChromosomes, binList, chromosomeGroupFile, breakSupportFile,
                                brokenChromosomeGroupFile)
        if inversionSupportFile:
            writeInversionSupportToFile(inversionSupport(adjMat, orderedChromosomes, binList,
                                                         _read_groups_quietly(chromosomeGroupFile)), inversionSupportFile)
        if refinedChromosomeOrderFile:
            refined, _log, _summary = refineOrdering(adjMat, orderedChromosomes, binList,
                                                     _read_groups_quietly(chromosomeGroupFile))
            writeScaffoldOrderingsToFile(refined, refinedChromosomeOrderFile)
        if junctionSupportFile or joinedFilesDirectory:
            junctionSupportToFiles(adjMat, orderedChromosomes, binList, chromosomeGroupFile, chromosomeOrderFile,
                                   plotOrderFile, junctionSupportFile, joinedFilesDirectory)
        if plotModule.plots_enabled(fullGenomePlot):                      # OG:700-707
            where = adjMat.bin_index(binList)
            rows = [where[b] for group in orderedChromosomes for s in group for b in s.binList]
            plotModule.plotContactMap(plotModule.DeviceImage(adjMat.ctx, 0, rows), resolution=resolution, tickCount=11,
                                      highlightChroms=getChromosomeOutlineCoords(orderedChromosomes), wInches=32,
                                      hInches=32, lP=2, hP=98, reverseColorMap='', showPlot=False,
                                      savePlot=fullGenomePlot, title=fullGenomePlotTitle, titleSuffix=False)
    finally:
        adjMat.ctx.close()
    print("Total run-time  for Part2 = " + str(time.time() - t0))
    print("- Part 2 (chromosome ordering) completed successfully")


def runResident(adjMat: GenomeMatrix, binList, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile,
                nScaffolds, scanScaffolds, resolution, savePlotDir=False, plotTitleSuffix=False, shard=None,
                chromosomeList=None, on_native_phase=None):
    """OG:691-709 on contacts that are already resident in HBM (what bench.py times).  ``binList``
    gives the bin of every row of the device matrix; bins that Part 1 did not assign to a group are
    simply never selected, which is what the reference's re-load restricted to grouped bins
    (OG:688-690) amounts to.  ``shard=(rank, world)``: see ``orderGenome``; every rank returns the whole order
    and rank 0 writes the two files.  ``chromosomeList``: the groups as readChromsFromFile would return them for
    chromosomeGroupFile (Part 1's ``DeviceMatrix.chromosome_groups``) when that file is still being written."""
    with paused_gc():
        if chromosomeList is None:
            chromosomeList = readChromsFromFile(chromosomeGroupFile)
        else:
            print("Chromosomes found " + str(len(chromosomeList)))
            print("Nodes found " + str(sum(len(c) for c in chromosomeList)))
        orderedChromosomes = orderGenome(adjMat, chromosomeList, binList, resolution, nScaffolds=nScaffolds,
                                         scanScaffolds=scanScaffolds, plotChrom=True, showPlot=False,
                                         savePlotDir=savePlotDir, plotTitleSuffix=plotTitleSuffix, shard=shard,
                                         on_native_phase=on_native_phase)
        tw = time.perf_counter()
        if shard is None or shard[0] == 0:
            text = orderGenome.file_text                        # formatted per chromosome beside the scans, or None
            writeScaffoldOrderingsToFile(orderedChromosomes, chromosomeOrderFile, None if text is None else [t[0] for t in text])
            writeBinIDsOrderingToFile([s for group in orderedChromosomes for s in group], plotOrderFile,
                                      None if text is None else [t[1] for t in text])
        if _PROFILE:
            sys.stderr.write("[hicmi] part2 files: %.1f ms\n" % ((time.perf_counter() - tw) * 1e3))
    return orderedChromosomes
