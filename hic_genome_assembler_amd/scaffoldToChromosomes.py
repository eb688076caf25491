"""Part 1 (bins -> chromosome groups) on MI355X: drop-in for the reference module of the same name.

Same ``runPipeline`` signature and intermediate files as /root/reference/HIC_ASSEMBLER/
scaffoldToChromosomes.py (S2C below), and the same stage-function names the reference's notebook
calls, but the N x N matrix lives in HBM behind a libhicmi context (``DeviceMatrix``) and every
heavy step is a hand-written gfx950 kernel reached through the C ABI of include/hicmi.h:

  S2C stage                                   here
  ------------------------------------------  ------------------------------------------------
  removeRows / row sums        S2C:100-136    hicmi_row_sums, hicmi_compact
  convertMatrix(distance)      S2C:138-155    fused into hicmi_upgma (k_build_w)
  squareform+average+dendrogram S2C:187-208   hicmi_upgma (k_nnchain + host label / leaf walk)
  reorderMatrix, similarity    S2C:157-163,149 fused into hicmi_rank_matrix (k_sort_rows)
  numpy.argsort[:, ::-1]       S2C:1132       hicmi_rank_matrix
  find_matrix_pvalue_breakpoints S2C:413-511  hicmi_cut_scan (+ host window logic)
  filter_noisy_breakpoints     S2C:553-727    hicmi_filter_scan (+ host control flow)
  hmmChromosomes (hmm = True)  S2C:730-942    hicmi_hmm_* (k_hmm.hip) + host control flow; opt-in: HICMI_HMM=1
  modularity_remaining_data    S2C:263-349    modularity.py; level 0 on hicmi_louvain_* (k_louvain.hip) with
                                              HICMI_LOUVAIN_DEVICE=1

Host control flow (loops over cut candidates, file formats, scaffold voting) is restated here in
Python because its decisions are sequential and tiny.  There is no CPU fallback for the kernels.

The HMM boundary finder (``hmm = True``, hmmlearn in the reference) is a seeded restatement of hmmlearn's 2-state
diagonal GaussianHMM, enabled by HICMI_HMM=1.  The Louvain tail (``modularity > 0``,
unseeded-random in the reference) is a seeded restatement in modularity.py.  The two Part 1 figures are drawn from the
device-resident matrix by plotContactMaps.py (exact percentiles, figure-resolution block means).
"""
from __future__ import annotations

import collections
import operator
import os
import sys
import time

import numpy as np

from . import _lib
from . import dist as _dist
from . import modularity as louvain
from . import plotContactMaps as plotModule
from .hostio import Bin, initiateLoci, paused_gc, read_contact_matrix, read_contact_matrix_cached  # noqa: F401  (re-exported reference names)


# ------------------------------------------------------------------------------------------------
class DeviceMatrix:
    """The contact map resident on one GPU, plus the host-side bookkeeping the reference keeps in
    its ``numpy.matrix`` / ``binList`` pair."""

    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx
        self.kind = "contacts"         # contacts -> distance -> similarity (labels only; transforms are fused)
        self.order = None              # current row/column order relative to the uploaded matrix
        self.np_sum = None
        self.seq_sum = None

    @property
    def n(self):
        return self.ctx.n

    def __len__(self):
        return self.ctx.n

    def hmm_states(self, c, p):
        """hmmChromosomes' model.fit(X) + model.predict(X) (S2C:796-801) for X = rows [c, n), columns [c, p) of the
        log-transformed similarity matrix in the current order."""
        if getattr(self, "hmm", None) is None:
            self.hmm = HmmDevice(self)
        return self.hmm.states(c, p)


class RankMatrix:
    """Device-resident result of ``argsort(axis=1)[:, ::-1]`` (S2C:1132) and its inverse."""

    def __init__(self, ctx: _lib.Context):
        self.ctx = ctx

    def __len__(self):
        return self.ctx.n

    def rows(self, row0=0, nrows=None):
        return self.ctx.rank_rows(row0, nrows, inverse=False)


def buildAdjacencyMatrix(matrixFile, binList, binID_dict=False, device=0, ctx=None):
    """S2C:70-98: dense matrix from HiC-Pro triplets, uploaded once to HBM."""
    cache = os.environ.get("HICMI_MATRIX_CACHE")           # "1": beside the text file; or a directory (hostio.py)
    host = read_contact_matrix_cached(matrixFile, binList, cache) if cache else read_contact_matrix(matrixFile, binList)
    ctx = ctx or _lib.Context(device)
    ctx.set_contacts(host)
    print("Rows in adjacency matrix " + str(len(binList)))
    return DeviceMatrix(ctx)


def removeRows(matrix: DeviceMatrix, binList, zeroRows=True, biasVals=False, store_row_sums=True):
    """S2C:100-136: drop rows (and columns) whose NumPy row sum is 0, then store each bin's
    left-to-right row sum.  ``biasVals`` filtering is kept for signature compatibility.
    ``store_row_sums=False``: the caller writes ``Bin.rowSum`` itself, later (``matrix.seq_sum`` holds the values;
    runResident does it beside the chain)."""
    np_sum, seq_sum = matrix.ctx.row_sums()
    first, world = getattr(matrix.ctx, "shard", (0, 1))
    if world > 1:                                          # one map over several GPUs: every rank summed its own rows
        np_sum = _dist.gather_owned(np_sum, 0, first, world)
        seq_sum = _dist.gather_owned(seq_sum, 0, first, world)
        matrix.ctx.set_row_sums(np_sum, seq_sum)
    dropped = np.zeros(len(binList), dtype=bool)
    if zeroRows is True:
        dropped |= np.asarray(np_sum) == 0
    if biasVals is not False:
        bias = np.fromiter((b.bias for b in binList), dtype=np.float64, count=len(binList))
        dropped |= ~dropped & ((bias > biasVals[1]) | (bias < biasVals[0]))
    print("Rows/columns to remove " + str(int(dropped.sum())))
    if dropped.any():
        keep = np.flatnonzero(~dropped).tolist()
        matrix.ctx.compact(keep)
        binList = [binList[i] for i in keep]
        np_sum, seq_sum = matrix.ctx.row_sums()
    matrix.np_sum, matrix.seq_sum = np_sum, seq_sum
    if store_row_sums:
        _store_row_sums(binList, seq_sum)
    return matrix, binList


def _store_row_sums(binList, seq_sum):
    for b, v in zip(binList, np.asarray(seq_sum, dtype=np.float64).tolist()):
        b.rowSum = v


def convertMatrix(adjacencyMatrix: DeviceMatrix, binList, distance=True, similarity=False):
    """S2C:138-155.  The transforms are elementwise and are fused into the kernels that consume
    them (k_build_w for distance, k_sort_rows for similarity), so this only records the stage."""
    if distance is True:
        adjacencyMatrix.kind = "distance"
    elif similarity is True:
        adjacencyMatrix.kind = "similarity"
    return adjacencyMatrix


def logTransformMatrix(matrix: DeviceMatrix, logBase=10, reverse=False):
    """S2C:165-183: log10(v + 1) of every non-zero cell (``reverse=True``: back again).  The device kernels that read
    the log-transformed similarity (k_hmm_obs, k_lv_graph) apply it themselves, so this only records the stage:
    similarity <-> log-similarity.  Other stages and bases are not supported."""
    if not isinstance(matrix, DeviceMatrix):
        raise TypeError("logTransformMatrix expects a DeviceMatrix")
    if logBase != 10:
        raise ValueError("logTransformMatrix supports logBase=10 only (got %r)" % (logBase,))
    frm, to = ("log-similarity", "similarity") if reverse else ("similarity", "log-similarity")
    if matrix.kind != frm:
        raise ValueError("logTransformMatrix(reverse=%r) expects the %s stage, not %s" % (reverse, frm, matrix.kind))
    matrix.kind = to
    return matrix


def averageClusterNodes(adjacencyMatrix: DeviceMatrix, nodeLabels, noPlot=True, meanwhile=None, want_ivl=True):
    """S2C:187-208: UPGMA + count-sorted leaf order.  Returns a dict with the two keys of SciPy's
    dendrogram object the reference uses ('ivl', 'leaves') plus the linkage matrix 'Z'.
    ``meanwhile``: host work that does not need the tree; it runs on this thread while the chain - one native call of
    ~100 ms that releases the interpreter lock - runs on another (``nodeLabels`` may then be a callable returning the
    labels: it is called after ``meanwhile``)."""
    t0 = time.time()
    if meanwhile is None:
        leaves, z = adjacencyMatrix.ctx.upgma(want_linkage=True)
    else:
        import threading
        box = {}

        def chain():
            try:
                box["out"] = adjacencyMatrix.ctx.upgma(want_linkage=True)
            except BaseException as exc:          # re-raised on the calling thread
                box["err"] = exc
        th = threading.Thread(target=chain)
        th.start()
        try:
            meanwhile()
        finally:
            th.join()
        if "err" in box:
            raise box["err"]
        leaves, z = box["out"]
    if callable(nodeLabels):
        nodeLabels = nodeLabels()
    print("Time to cluster " + str(time.time() - t0))
    leaves = np.asarray(leaves).tolist()
    return {"ivl": [nodeLabels[i] for i in leaves] if want_ivl else None, "leaves": leaves, "Z": z}


def dendrogramLeafOrder_toFile(dendrogramObj, outFile, lines=None):
    """S2C:210-220: ``label<TAB>leaf`` lines, no trailing newline.  ``lines``: the line of every leaf, indexed by leaf
    (formatted beside the chain: runResident)."""
    with open(outFile, "w") as fh:
        if lines is not None:
            fh.write("\n".join(map(lines.__getitem__, dendrogramObj["leaves"])))
        else:
            fh.write("\n".join(l + "\t" + str(i) for l, i in zip(dendrogramObj["ivl"], dendrogramObj["leaves"])))


def readDengrogramLeavesFromFile(dendrogramFile):
    """S2C:222-234."""
    out = {"ivl": [], "leaves": []}
    with open(dendrogramFile) as fh:
        for line in fh:
            cols = line.strip("\r").strip("\n").split("\t")
            out["ivl"].append(cols[0])
            out["leaves"].append(int(cols[-1]))
    return out


def reorderMatrix(matrix: DeviceMatrix, binList, newOrder):
    """S2C:157-163: the permutation is applied by the consuming kernel through an index vector."""
    newOrder = np.asarray(newOrder, dtype=np.int64).tolist()
    matrix.order = newOrder if matrix.order is None else [matrix.order[i] for i in newOrder]
    return matrix, [binList[i] for i in newOrder]


def rankOrderMatrix(matrix: DeviceMatrix) -> RankMatrix:
    """S2C:1132 ``numpy.asarray(numpy.argsort(adjMat, axis=1)[:, ::-1])`` on the similarity matrix
    in the current order.  Ties (undefined in the reference) resolve to the larger column first."""
    if matrix.kind != "similarity":
        raise ValueError("rankOrderMatrix expects the similarity stage (call convertMatrix(similarity=True))")
    order = matrix.order if matrix.order is not None else list(range(matrix.n))
    matrix.ctx.rank_matrix(order)
    return RankMatrix(matrix.ctx)


# ------------------------------------------------------------------------------------------------
def hyper_geom(x, M, n, N):
    """S2C:352-368 (= scipy.stats.hypergeom.sf(x-1, M, n, N)), evaluated by libhicmi."""
    return _lib.hypergeom_sf(x, M, n, N)


def _window_scores(input_array, window_size):
    """break_sigs of S2C:390-400 as an int64 array (None for the ["NA","NA","NA"] case, S2C:380-381)."""
    if window_size >= len(input_array):
        return None
    a = np.asarray(input_array, dtype=np.int64)
    h = int(window_size)
    cs = np.concatenate(([0], np.cumsum(a)))
    scores = np.zeros(len(a) - h, dtype=np.int64)
    full = max(0, len(a) - 2 * h + 1)                 # windows whose right half is complete; the rest score 0
    if full:
        scores[:full] = (cs[h:h + full] - cs[:full]) - (cs[2 * h:2 * h + full] - cs[h:h + full])
    return scores


def get_sliding_window_distance_metrics(input_array, window_size, global_index=0):
    """S2C:370-411: left-half minus right-half window sums; 0 where the right half is short."""
    scores = _window_scores(input_array, window_size)
    if scores is None:
        return ["NA", "NA", "NA"]
    best = int(np.flatnonzero(scores == scores.max())[0])
    return [int(v) for v in scores], int(window_size), best


def _device_scan_loops(ctx):
    """The scan loops run with their control flow on the device when the context has the whole rank matrix (one GPU)
    and offers the entry points; HICMI_HOST_SCANS=1 keeps the per-scan host loops (the A/B, and what a row shard uses)."""
    if os.environ.get("HICMI_HOST_SCANS"):
        return False
    _first, world = getattr(ctx, "shard", (0, 1))
    return world == 1 and hasattr(ctx, "first_pass_cuts") and hasattr(ctx, "filter_cuts")


def find_matrix_pvalue_breakpoints(argsorted_mat: RankMatrix, start, min_size, world_size, psig=.05):
    """S2C:413-511 for one ``start``.  Counts and significance flags come from the GPU
    (hicmi_cut_scan); the >= 90 % rule that shrinks M (S2C:473-483) and the window scan run here.
    The window-shrinking retry of S2C:499-508 cannot produce a cut (its scores are < min_size while
    S2C:488 tests == min_size), so it is not repeated."""
    ctx = argsorted_mat.ctx
    first, world = getattr(ctx, "shard", (0, 1))
    M = world_size
    loop_count = 0
    while True:
        sig = ctx.cut_scan(int(start), int(M), float(psig))
        if world > 1:                                      # flags of this rank's rows -> all rows (one all-gather per scan)
            sig = _dist.gather_owned(sig, int(start), first, world)
        loop_count += 1
        if (int(sig.sum()) / len(sig)) >= .9:
            morg = M
            M = int(M - start)
            print("- M value (world_size) changed to dynamic {} --> {}".format(morg, M))
        else:
            break
        if loop_count >= 5:
            break
    scores = _window_scores(sig, min_size)
    if scores is None:
        return [], []
    inds = [int(v) for v in np.flatnonzero(scores == min_size) + min_size]         # S2C:488
    return [min_size] * len(inds), inds


def pre_process_all_matrix_breakpoints(argsorted_mat: RankMatrix, min_size=5, min_frac=.05, psig=.05):
    """S2C:513-551.  As in the reference the scan tests against the literal .05 (S2C:535), not
    the ``psig`` argument."""
    mat_size = len(argsorted_mat)
    stop_ind = int(mat_size - (mat_size * min_frac))
    ind = 0
    cinds = []
    if min_frac == 1:
        return cinds
    if _device_scan_loops(argsorted_mat.ctx) and min_size >= 1:
        # the same loop with its decisions on the device (hicmi_first_pass_cuts): one host round trip per batch of scans
        cinds, m_changes = argsorted_mat.ctx.first_pass_cuts(min_size, stop_ind, .05)
        print("\n".join(first_pass_report(cinds, m_changes)))
        return cinds
    while True:
        _vals, pre_cut_inds = find_matrix_pvalue_breakpoints(argsorted_mat, ind, min_size, mat_size - ind, psig=.05)
        if len(pre_cut_inds) == 0:
            break
        ind += pre_cut_inds[0]
        cinds.append(ind)
        if (ind >= stop_ind) or ((mat_size - ind) <= min_size):
            break
    print("- Breakpoints found {}".format(len(cinds)))
    return cinds


def first_pass_report(cinds, m_changes):
    """The lines pre_process_all_matrix_breakpoints prints, from the device loop's results (cuts, M changes)."""
    return ["- M value (world_size) changed to dynamic {} --> {}".format(morg, m) for morg, m in m_changes] + \
        ["- Breakpoints found {}".format(len(cinds))]


def filter_report(original_inds, out, warned):
    """The lines filter_noisy_breakpoints prints, from the device loop's results (kept cuts, warnings)."""
    return ["- WARNING - Maximum number of rounds {} exceeded".format(10 * len(original_inds))] * warned + \
        ["- Original cut indices {}".format(list(original_inds)), "- Filtered cut indices {}".format(out)]


def filter_noisy_breakpoints(argsorted_mat: RankMatrix, original_inds, psig=.05):
    """S2C:553-727.  Row tests run on the GPU (hicmi_filter_scan); the merge decisions between
    candidate cuts are scalar hypergeometric tests evaluated by libhicmi's host code."""
    if len(original_inds) == 0:
        return []
    ctx = argsorted_mat.ctx
    first, world = getattr(ctx, "shard", (0, 1))
    n = len(argsorted_mat)
    ascending = all(b > a for a, b in zip(original_inds, original_inds[1:]))
    if _device_scan_loops(ctx) and ascending and 0 <= original_inds[0] and original_inds[-1] < n:
        out, warned = ctx.filter_cuts(original_inds, psig)          # the loops below, on the device (hicmi_filter_cuts)
        print("\n".join(filter_report(original_inds, out, warned)))
        return out
    MD = int(n / 5)
    MAX_ROUNDS = 10 * len(original_inds)
    altered = [int(v) for v in original_inds]
    prev_filtered = {}
    while True:
        start = 0
        filtered = {}
        round_count = 0
        while True:
            if round_count >= MAX_ROUNDS:
                print("- WARNING - Maximum number of rounds {} exceeded".format(MAX_ROUNDS))
                break
            M = n - start
            noise_found = 0
            keep_from = 0
            for i, c in enumerate(altered):
                local = c - start
                n_rows = min(n - start, MD + 1)            # rows beyond start+MD are forced to 0 (S2C:626-628)
                flags = np.zeros(n - start, dtype=np.int64)
                own = ctx.filter_scan(start, c, n_rows, M, float(psig))
                flags[:n_rows] = _dist.gather_owned(own, start, first, world) if world > 1 else own
                sig_cuts = []
                fc_prev = start
                for ai_ind, ai in enumerate(altered):
                    if ai == fc_prev:
                        continue
                    lo, hi = fc_prev, ai
                    fc_prev = ai
                    if hi <= lo:
                        break
                    x = int(flags[lo - start:hi - start].sum())
                    noise_pval = hyper_geom(x, M, local, hi - lo)
                    if noise_pval < psig:
                        sig_cuts.append((ai_ind, ai))
                if sig_cuts:
                    keep_from, start = sig_cuts[-1]
                    filtered[start] = ''
                    noise_found = 1
                    break
                filtered[c] = ''
                keep_from = i
            round_count += 1
            if noise_found == 0:
                break
            altered = altered[keep_from:]
        if prev_filtered != filtered:
            altered = sorted(filtered)
            prev_filtered = filtered
        else:
            break
    out = sorted(filtered.keys())
    print("- Original cut indices {}".format(list(original_inds)))
    print("- Filtered cut indices {}".format(out))
    return out


# ------------------------------------------------------------------------------------------------
def _louvain_tail(adjMat: DeviceMatrix, binList, cutIndices, n_rounds):
    """modularity.modularity_remaining_data on the bins after the last cut index: (new_order, cutIndices).  With
    HICMI_LOUVAIN_DEVICE=1 the graph is built on the device from the resident matrix and level 0 runs there; otherwise
    the tail's similarity comes down and the host restatement runs."""
    start = sorted(cutIndices)[-1] if len(cutIndices) else 0
    order = adjMat.order if adjMat.order is not None else list(range(adjMat.n))
    tail_rows = list(order[start:])
    if louvain.louvain_device_enabled():
        adjMat.ctx.louvain_graph(tail_rows)
        return louvain.modularity_remaining_data(None, binList, cutIndices, n_rounds=n_rounds, ctx=adjMat.ctx)
    sim_tail = adjMat.ctx.plot_downsample(2, tail_rows, len(tail_rows))
    return louvain.modularity_remaining_data(louvain.log_transform(sim_tail), binList, cutIndices, n_rounds=n_rounds)


def modularity_remaining_data(adjacencyMatrix: DeviceMatrix, binList, cutIndices, n_rounds=20):
    """S2C:263-349: partition the bins after the last cut index by modularity (the best of ``n_rounds`` Louvain runs)
    and reorder that tail by community, largest first.  ``adjacencyMatrix``: a DeviceMatrix at its log-similarity stage
    (logTransformMatrix).  Returns (adjacencyMatrix, binList, cutIndices), both reordered, as the reference does."""
    if not isinstance(adjacencyMatrix, DeviceMatrix) or adjacencyMatrix.kind != "log-similarity":
        raise ValueError("modularity_remaining_data expects a DeviceMatrix at its log-similarity stage "
                         "(convertMatrix(similarity=True), then logTransformMatrix)")
    new_order, cutIndices = _louvain_tail(adjacencyMatrix, binList, cutIndices, n_rounds)
    adjacencyMatrix, binList = reorderMatrix(adjacencyMatrix, binList, new_order)
    return adjacencyMatrix, binList, cutIndices


# ------------------------------------------------------------------------------------------------
# HMM boundary finder (hmm = True, S2C:730-942).  hmmlearn's GaussianHMM(n_components=2, covariance_type="diag",
# n_iter=1000, init_params="cm", params="cmt") restated from its formulas (not checked against hmmlearn itself, which
# is not a dependency): the passes over X run on the device (k_hmm.hip), the k-means++ draws, the restarts and the
# convergence tests here.  sklearn's unseeded KMeans(n_init=10) is replaced by seeded k-means++ (HICMI_HMM_SEED).
HMM_N_ITER, HMM_TOL, HMM_MIN_COVAR = 1000, 1e-2, 1e-3
HMM_KMEANS_RESTARTS, HMM_KMEANS_MAX_ITER, HMM_KMEANS_TOL = 10, 300, 1e-4
# S2C:797-799: the reference sets model.startmat_ (misspelled, never read) - hmmlearn starts from a uniform startprob_,
# and params has no 's', so it stays uniform
HMM_STARTPROB = (.5, .5)
HMM_TRANSMAT = ((.9, .1), (.0001, .9999))


def hmm_enabled():
    """The HMM path is opt-in: its parity with the reference is statistical (seeded initialisation)."""
    return os.environ.get("HICMI_HMM", "") == "1"


class HmmDevice:
    """Fits and decodes the HMM of one (c, p) window of a DeviceMatrix.  X is built on the device once per boundary
    at its widest D; narrower rounds of the same boundary read a column prefix of it."""

    def __init__(self, matrix: DeviceMatrix, seed=None):
        self.matrix = matrix
        self.seed = int(os.environ.get("HICMI_HMM_SEED", "0")) if seed is None else int(seed)
        self.fit_index = 0
        self.built = None                       # (c, width) of the X on the device
        self.profile = os.environ.get("HICMI_HMM_PROFILE") == "1"
        self.stats = collections.Counter()

    def _tick(self, key, t0):
        self.stats[key + "_ms"] += (time.perf_counter() - t0) * 1e3

    def states(self, c, p):
        ctx = self.matrix.ctx
        n = self.matrix.n
        D = p - c
        t0 = time.perf_counter()
        if self.built is None or self.built[0] != c or self.built[1] < D:
            order = self.matrix.order if self.matrix.order is not None else list(range(n))
            ctx.hmm_load_obs(order, c, p)
            self.built = (c, D)
            self.stats["builds"] += 1
        ctx.hmm_set_width(D)
        self._tick("obs", t0)
        T = n - c
        t0 = time.perf_counter()
        means, covars = hmm_init_params(ctx, T, self.seed, self.fit_index, self.stats)
        self._tick("init", t0)
        t0 = time.perf_counter()
        means, covars, transmat, hist = ctx.hmm_fit(HMM_STARTPROB, means, covars, HMM_TRANSMAT, HMM_N_ITER, HMM_TOL)
        self._tick("fit", t0)
        t0 = time.perf_counter()
        st = ctx.hmm_decode(HMM_STARTPROB, means, covars, transmat)
        self._tick("decode", t0)
        self.fit_index += 1
        self.stats["fits"] += 1
        self.stats["em_iterations"] += len(hist)
        if self.profile:
            sys.stderr.write("[hicmi] hmm fit %d: X %d x %d, %d EM iterations, logprob %.6f\n"
                             % (self.fit_index, T, D, len(hist), hist[-1]))
        return st

    def report(self):
        s = self.stats
        sys.stderr.write("[hicmi] hmm: %d fits, %d EM iterations, %d k-means iterations, %d X builds; ms: obs %.1f, "
                         "init (k-means) %.1f, fit %.1f, decode %.1f\n"
                         % (s["fits"], s["em_iterations"], s["kmeans_iterations"], s["builds"], s["obs_ms"],
                            s["init_ms"], s["fit_ms"], s["decode_ms"]))


def hmm_init_params(ctx, T, seed, fit_index, stats=None):
    """GaussianHMM._init with init_params="cm" on the X of ``ctx``: means from the best of 10 seeded k-means++ / Lloyd
    restarts (lowest inertia, the first on a tie; numpy.random.default_rng([seed, fit_index, restart])), covariances
    diag(numpy.cov(X.T)) + min_covar for both states."""
    mean, m2 = ctx.hmm_col_stats()
    var1 = m2 / (T - 1)
    tol = HMM_KMEANS_TOL * float(np.mean(m2 / T))             # sklearn: tol * mean(var(X, axis=0))
    best = None
    for restart in range(HMM_KMEANS_RESTARTS):
        rng = np.random.default_rng([seed, fit_index, restart])
        rows = kmeans_plusplus_rows(T, ctx.hmm_dist2, rng)
        init = np.vstack([ctx.hmm_get_obs(r, 1) for r in rows])
        centers, _labels, inertia, n_iter = ctx.hmm_kmeans(init, HMM_KMEANS_MAX_ITER, tol, want_labels=False)
        if stats is not None:
            stats["kmeans_iterations"] += n_iter
        if best is None or inertia < best[1]:
            best = (centers, inertia)
    covars = np.vstack([var1 + HMM_MIN_COVAR, var1 + HMM_MIN_COVAR])
    return best[0], covars


def kmeans_plusplus_rows(T, dist2, rng):
    """sklearn's greedy k-means++ for 2 clusters (2 + int(log 2) = 2 local trials): the rows of X chosen as the initial
    centers.  ``dist2(rows)``: squared distances of every row of X to the given rows (len(rows) x T)."""
    first = int(rng.integers(T))
    closest = dist2([first])[0]
    pot = closest.sum()
    rand_vals = rng.uniform(size=2) * pot
    cand = np.minimum(np.searchsorted(np.cumsum(closest), rand_vals), T - 1)
    dist = np.minimum(closest, dist2(cand))
    best = int(np.argmin(dist.sum(axis=1)))
    return [first, int(cand[best])]


def identifyBoundry(hiddenStates, cutIndices, switchCount=10):
    """S2C:730-752: the start state is the majority of the first switchCount states (a tie: state 0); the boundary is
    the first window of switchCount states with no start state, over the windows range(0, len - switchCount)."""
    states = np.asarray(hiddenStates).astype(np.int64)
    head = states[0:switchCount]
    ones = int((head == 1).sum())
    startState = 1 if ones > len(head) - ones else 0
    n_win = len(states) - switchCount
    if n_win <= 0:
        return 0
    other = np.concatenate(([0], np.cumsum(states != startState)))
    full = np.flatnonzero(other[switchCount:switchCount + n_win] - other[:n_win] == switchCount)
    return int(full[0]) + cutIndices[-1] if len(full) else 0


# hmmChromosomes / identifyChromosomeGroupsHMM (S2C:754-942) as generators: every ``adjacencyMatrix.hmm_states(c, p)``
# becomes ``states = yield (c, width, fit_index)`` with width = p - c, every print a call of ``emit``.  fit_index counts
# the fits of one run from 0, as HmmDevice.fit_index does.  identifyChromosomeGroupsHMM drives them with a matrix and
# print; the HMM sweep (sweepHMM.py) drives the generators of many settings in lock step.
def hmm_chromosomes_steps(n, cutIndices, minSize, convergenceRounds, lookAhead, counter, emit):
    """S2C:754-819 on an n-bin matrix."""
    if lookAhead != False:                                  # noqa: E712  (the reference's test: 0.0 means "all")
        lookAhead = int((float(n - cutIndices[-1]) * lookAhead) + cutIndices[-1])
    else:
        lookAhead = n
    prevCutInd, roundCount = lookAhead, 1
    while roundCount <= convergenceRounds:
        if (n - cutIndices[-1]) / 2 < minSize:
            cutInd = prevCutInd
            cutIndices.append("NA")
            break
        c = cutIndices[-1]
        width = max(0, min(prevCutInd, n) - c)                 # len(X[0]) of r[c:prevCutInd]
        emit("Input matrix size = " + str(n - c) + " x " + str(width))
        emit("HMM round = " + str(roundCount))
        if width < minSize:
            cutInd = lookAhead
        else:
            hiddenStates = yield (c, width, counter[0])
            counter[0] += 1
            cutInd = identifyBoundry(hiddenStates, cutIndices, switchCount=minSize)
        if cutInd != prevCutInd:
            prevCutInd = cutInd
            roundCount += 1
            continue
        else:
            emit("HMM convergence rounds = " + str(roundCount))
            cutIndices.append(int(cutInd))
            break
    if roundCount > convergenceRounds:
        cutIndices.append(int(cutInd))
        emit("WARNING... HMM failed to converge after " + str(roundCount) + " rounds...")
        emit("Proceeding with last found cutIndex of " + str(cutInd) + "...")
    return cutIndices


def hmm_groups_steps(n, minSize=5, modularity=.05, convergenceRounds=5, lookAhead=.2, louvainRounds=20,
                     prev_cutInds=False, emit=print, counter=None, clock=time.time):
    """identifyChromosomeGroupsHMM on an n-bin matrix; yields fit requests (c, width, fit_index), is sent the decoded
    states, and returns the cut indices."""
    counter = [0] if counter is None else counter
    emit("#########################" + '\n' + "#########################")
    emit("Working on iterative 2 state HMMs to identify chromosome boundaries...")
    startTime = clock()
    matrixLength = float(n)
    remainder = matrixLength - (modularity * matrixLength)
    cutIndices = [0]
    if modularity == 1:
        return []
    if prev_cutInds is not False:
        cutIndices = prev_cutInds
    while cutIndices[-1] <= remainder:
        emit("#########################" + '\n' + "#########################")
        cutIndices = yield from hmm_chromosomes_steps(n, cutIndices, minSize, convergenceRounds, lookAhead, counter, emit)
        emit("Cut indices =  " + str(cutIndices))
        if cutIndices[-1] == 0:
            emit("Algorithm terminated. No obvious chromome boundry could be found... ")
            break
        if cutIndices[-1] == "NA":
            cutIndices.pop(-1)
            break
    if cutIndices[0] == 0:
        cutIndices.pop(0)
    emit("#########################" + '\n' + "#########################")
    emit("HMM rounds completed in " + str(clock() - startTime) + " seconds")
    emit("Chromosome groups found via HMMs " + str(len(cutIndices)) + " / " + str(len(cutIndices) + 1))
    if len(cutIndices) == 0:
        emit("- WARNING - no chromosome boundary found by the HMMs (the reference raises IndexError here)")
        return []
    if cutIndices[-1] == n:
        emit("- WARNING - Last cut index found to be length of current matrix removing index values of {}".format(cutIndices[-1]))
        cutIndices.pop(-1)
        if len(cutIndices) == 0:
            emit("- WARNING - no chromosome boundary left (the reference raises IndexError here)")
            return []
        if (n - cutIndices[-1]) >= (5 * (n * modularity)):
            emit("- convergenceRounds reduced from {} --> {}".format(convergenceRounds, convergenceRounds - 1))
            if convergenceRounds - 1 == 0:
                emit("- Failed to converge after reducing convergence rounds all the way to 1... Returning current indices")
                return cutIndices
            else:
                emit("- Recursing on identifyChromosomeGroupsHMM function, due to remaining fraction of data being greater "
                     "than 5x than that of desired fraction")
                cutIndices = yield from hmm_groups_steps(n, minSize=5, modularity=.05,
                                                         convergenceRounds=convergenceRounds - 1, lookAhead=.5,
                                                         louvainRounds=20, prev_cutInds=cutIndices, emit=emit,
                                                         counter=counter, clock=clock)
    emit("Total time to identify chromosome boundries = " + str(clock() - startTime) + " seconds")
    return cutIndices


def drive(gen, states_of):
    """Run one generator to its end with ``states_of(c, width, fit_index)`` serving its requests; returns its result."""
    try:
        req = next(gen)
        while True:
            req = gen.send(states_of(*req))
    except StopIteration as stop:
        return stop.value


def identifyChromosomeGroupsHMM(adjacencyMatrix, binList, minSize=5, modularity=.05, convergenceRounds=5, lookAhead=.2,
                                louvainRounds=20, prev_cutInds=False):
    """S2C:868-942.  ``adjacencyMatrix``: the DeviceMatrix at its similarity stage (its ``hmm_states(c, p)`` fits and
    decodes X = log10(similarity + 1)[c:n, c:p]).  One documented difference: where the reference raises IndexError
    (no cut left after the leading 0 is popped, S2C:920), this returns [] with a warning."""
    steps = hmm_groups_steps(len(adjacencyMatrix), minSize=minSize, modularity=modularity,
                             convergenceRounds=convergenceRounds, lookAhead=lookAhead, louvainRounds=louvainRounds,
                             prev_cutInds=prev_cutInds, emit=print)
    return drive(steps, lambda c, width, _fit_index: adjacencyMatrix.hmm_states(c, c + width))


# ------------------------------------------------------------------------------------------------
def _bin_line(b):
    return f"{b.ID}\t{b.chrom}\t{b.start}\t{b.stop}\t{b.bias}"


def writeBinGroupingsToFile(coords, binList, outFile, bin_lines=None):
    """S2C:945-964.  Returns the groups as lists of the lines written (what
    readBinGroupingsFromFile gives back for this file).  ``bin_lines``: {bin ID: its line} when the caller has formatted
    them already (runResident does, beside the chain)."""
    bounds = [0] + [int(c) for c in coords] + [len(binList)]
    groups, text = [], []
    for g in range(len(bounds) - 1):
        if bin_lines is not None:
            lines = [bin_lines[b.ID] for b in binList[bounds[g]:bounds[g + 1]]]
        else:
            lines = [_bin_line(b) for b in binList[bounds[g]:bounds[g + 1]]]
        text.append("### Chromosome group " + str(g + 1) + " ###\n")
        if lines:
            text.append("\n".join(lines) + "\n")
        groups.append(lines)
    with open(outFile, "w") as fh:
        fh.write("".join(text))
    return groups


def readSizeFileToDict(sizeFile):
    """S2C:968-979."""
    sizes = {}
    with open(sizeFile) as fh:
        for line in fh:
            cols = line.strip("\r").strip("\n").split("\t")
            sizes[cols[0]] = int(cols[1])
    return sizes


def readBinGroupingsFromFile(binGroupingsFile):
    """S2C:981-999: first line skipped unconditionally, every later '#' line starts a new group."""
    groups, cur = [], []
    with open(binGroupingsFile) as fh:
        fh.readline()
        for line in fh:
            line = line.strip("\n").strip("\r")
            if line[0] != "#":
                cur.append(line)
            else:
                groups.append(cur)
                cur = []
    groups.append(cur)
    print(str(len(groups)) + " chromosomes read in from file")
    return groups


def _assess_rows(pairs, scaffDict, percentToAssign):
    """The decisions of assessClusterList on (bin, scaffold) pairs: (rows of the report - scaffold, bins here, bins in
    all, percentage -, the bins of the scaffolds assigned, their names, bins of the others)."""
    members = collections.Counter(map(_second, pairs))       # (a dict: scaffolds in order of first appearance)
    rows, final, names, false_pos = [], [], [], 0
    for s, have in members.items():
        total = len(scaffDict[s])
        pct = round(((float(have) / float(total)) * 100.), 2)
        rows.append((s, have, total, pct))
        if pct >= percentToAssign:
            final += scaffDict[s]
            names.append(s)
        else:
            false_pos += have
    return rows, final, names, false_pos


def _assess_text(rows, assigned, out):
    out.append("#Scaffold\tNodesAssigend\tTotalNodes\tAssigned%\n")
    for s, have, total, pct in rows:
        out.append(str(s) + "\t" + str(have) + "\t" + str(total) + "\t" + str(pct) + "%\n")
    out.append("Total scaffolds clustered to chromosome " + str(len(rows)) + "\n")
    out.append("Total scaffolds assigned to chromosome " + str(assigned) + "\n")


def _assess_group(pairs, scaffDict, out, percentToAssign):
    """assessClusterList on (bin, scaffold) pairs; ``out`` collects the report lines."""
    rows, final, names, false_pos = _assess_rows(pairs, scaffDict, percentToAssign)
    _assess_text(rows, len(names), out)
    return final, false_pos, len(names)


_second = operator.itemgetter(1)


class PairList(list):
    """A group that is known to hold (bin, scaffold) pairs only (_bin_group_pairs): _pairs_of_lines passes it through."""


def _pairs_of_lines(cList):
    """(bin, scaffold) of every bin-grouping line; entries that already are such pairs pass through."""
    if isinstance(cList, PairList):
        return cList
    return [line if isinstance(line, tuple) else tuple(line.split("\t", 2)[:2]) for line in cList]


def _bin_pairs(binList):
    """{bin ID: (bin ID text, scaffold)} - independent of the grouping, so runResident builds it beside the chain."""
    return {b.ID: (str(b.ID), b.chrom) for b in binList}


def _bin_group_pairs(coords, binList, pairs=None):
    """What readBinGroupingsFromFile + the split in assessChromosomeClustering extract from the bin-grouping file:
    per group the (bin ID text, scaffold) pairs - taken from the bins themselves (``pairs``: _bin_pairs of them)."""
    bounds = [0] + [int(c) for c in coords] + [len(binList)]
    if pairs is None:
        return [PairList((str(b.ID), b.chrom) for b in binList[bounds[g]:bounds[g + 1]]) for g in range(len(bounds) - 1)]
    ids = [b.ID for b in binList]
    return [PairList(map(pairs.__getitem__, ids[bounds[g]:bounds[g + 1]])) for g in range(len(bounds) - 1)]


def assessClusterList(cList, scaffDict, outFile, percentToAssign=51.):
    """S2C:1001-1036: a scaffold joins the group holding >= 51 % of its bins and brings ALL its bins."""
    out = []
    res = _assess_group(_pairs_of_lines(cList), scaffDict, out, percentToAssign)
    outFile.write("".join(out))
    return res


def _write_text(path, text):
    with open(path, "w") as fh:
        fh.write(text)


def _scaffold_bins(pairs):
    """{scaffold: [[bin, scaffold], ...] with the bins ascending} over (bin, scaffold) pairs (S2C:1043-1053)."""
    scaffolds = {}
    for bin_id, scaff in pairs:
        scaffolds.setdefault(scaff, []).append(int(bin_id))
    return {s: [[b, s] for b in sorted(ids)] for s, ids in scaffolds.items()}


def assessChromosomeClustering(chromList, statsFile, percentToAssign=51., write=None, scaffolds=None):
    """S2C:1038-1077.  ``chromList``: groups of bin-grouping lines (``ID<TAB>scaffold<TAB>...``).  ``write``: called as
    ``write(fn, *args)`` to put the report on disk (default: at once).  ``scaffolds``: the scaffold -> bins table when
    the caller has built it already (it does not depend on the grouping: every bin is in exactly one group)."""
    groups = [_pairs_of_lines(grp) for grp in chromList]
    if scaffolds is None:
        scaffolds = _scaffold_bins(p for grp in groups for p in grp)
    final, false_pos, assigned, per_group = GroupList(), 0, 0, []
    for grp in groups:
        rows, nodes, names, fp = _assess_rows(grp, scaffolds, percentToAssign)
        per_group.append((rows, len(names)))
        if len(nodes) > 0:
            final.append(nodes)
            final.scaffolds.append(names)
        false_pos += fp
        assigned += len(names)
    total = sum(len(grp) for grp in groups)

    def report():
        """The text of the file (formatted where it is written: on the writer thread when ``write`` defers it)."""
        out = []
        for k, (rows, n_assigned) in enumerate(per_group):
            out.append("### Chromosome" + str(k + 1) + " ###\n")
            _assess_text(rows, n_assigned, out)
            out.append("####################\n")
        out.append("Total Nodes " + str(total) + "\n")
        out.append("Properly clustered nodes " + str(total - false_pos) + "\n")
        out.append("Falsely clustered nodes " + str(false_pos) + "\n")
        out.append("Total scaffolds assigned to chromosomes " + str(assigned) + "\n")
        out.append("Error rate ~" + str(round((float(false_pos) / float(total)) * 100., 2)) + "%\n")
        _write_text(statsFile, "".join(out))
    if write is None:
        report()
    else:
        write(report)
    return final


class GroupList(list):
    """assessChromosomeClustering's result: the groups' [bin, scaffold] entries, and beside them (``scaffolds``) the names of
    the scaffolds of every group - what rankChromosomeGroups would otherwise collect from all the entries again."""

    def __init__(self, *a):
        super().__init__(*a)
        self.scaffolds = []


def rankChromosomeGroups(chromList, scaffSizeDict):
    """The order in which S2C:1079-1100 writes the groups: by total scaffold bp, largest first (stable).  What
    orderGenome.readChromsFromFile gives back for the file written from it."""
    names = getattr(chromList, "scaffolds", None)
    if names is not None and len(names) == len(chromList):
        sizes = [sum(scaffSizeDict[s] for s in grp_names) for grp_names in names]
    else:
        sizes = [sum(scaffSizeDict[s] for s in {e[1]: '' for e in grp}) for grp in chromList]
    ranked = sorted(range(len(chromList)), key=lambda k: sizes[k], reverse=True)
    return [chromList[k] for k in ranked]


def writeChromosomeGroupingsToFile(chromList, scaffSizeDict, outFile, entry_lines=None):
    """S2C:1079-1100: groups ordered by total scaffold bp, largest first (stable).  ``entry_lines``: {bin ID: its
    ``bin<TAB>scaffold`` line with the newline} when formatted already."""
    text = []
    for new_id, grp in enumerate(rankChromosomeGroups(chromList, scaffSizeDict)):
        text.append("### Chromosome group " + str(new_id + 1) + " ###\n")
        if entry_lines is not None:
            text.extend([entry_lines[e[0]] for e in grp])
        else:
            text.extend(str(e[0]) + "\t" + str(e[1]) + "\n" for e in grp)
    with open(outFile, "w") as fh:
        fh.write("".join(text))


# ------------------------------------------------------------------------------------------------
# Group support: the contacts' own evidence for the scaffold vote of assessChromosomeClustering.
def readScaffoldBinCounts(hicProBedFile):
    """{scaffold: number of bins in the bed}, in order of first appearance (bins with a NaN bias included)."""
    counts = {}
    with open(hicProBedFile) as fh:
        for line in fh:
            name = line.split("\t", 1)[0]
            counts[name] = counts.get(name, 0) + 1
    return counts


def _run_lengths(labels):
    """'3:12,7:9' for 12 labels '3' followed by 9 labels '7'; 'NA' for none."""
    out, k = [], 0
    while k < len(labels):
        j = k + 1
        while j < len(labels) and labels[j] == labels[k]:
            j += 1
        out.append(labels[k] + ":" + str(j - k))
        k = j
    return ",".join(out) if out else "NA"


def groupSupport(matrix, binList, chromList, scaffoldBins, minRatio=3.0):
    """One record per scaffold of ``scaffoldBins`` ({scaffold: bins in the bed}, bed order): how densely its bins touch
    every chromosome group of ``chromList`` (orderGenome.readChromsFromFile's groups) in the resident map whose rows are
    ``binList``, zero rows compacted away or not.  The sums come from the device (hicmi_group_sums).

    Record: scaffold, bins, live_bins (present with a non-zero row), assigned / best / second (group indices or None),
    best_density, second_density, ratio, verdict (supported, contested, rescued, ambiguous, no_contacts), runs (the
    per-bin best group, run-length encoded with 1-based group numbers), density (one value per group), live_ids."""
    names = list(scaffoldBins)
    sid = {name: k for k, name in enumerate(names)}
    n, G, S = len(binList), len(chromList), len(names)
    if G < 1 or n != matrix.ctx.n:
        raise ValueError("groupSupport needs at least one group and the bins of the matrix rows")
    ids = np.fromiter((b.ID for b in binList), dtype=np.int64, count=n)
    scaf = np.fromiter((sid[b.chrom] for b in binList), dtype=np.int32, count=n)
    np_sum = getattr(matrix, "np_sum", None)
    if np_sum is None or len(np_sum) != n:
        np_sum = matrix.ctx.row_sums()[0]
    live = np.asarray(np_sum) != 0
    label = {int(e[0]): g for g, group in enumerate(chromList) for e in group}
    grp = np.fromiter((label.get(i, -1) for i in ids.tolist()), dtype=np.int32, count=n)
    grp[~live] = -1                                        # a label on a zero row is ignored: compaction changes nothing
    binsum, scafsum = matrix.ctx.group_sums(grp, scaf, G, S, want_bins=True)
    labelled = grp >= 0
    m = np.bincount(grp[labelled], minlength=G).astype(np.int64)
    own = np.zeros((S, G), dtype=np.int64)
    np.add.at(own, (scaf[labelled], grp[labelled]), 1)
    L = np.bincount(scaf[live], minlength=S).astype(np.int64)
    pairs = L[:, None] * (m[None, :] - own)
    density = np.divide(scafsum, pairs, out=np.zeros_like(scafsum), where=pairs != 0)
    by_id = np.argsort(ids, kind="stable")
    bins_of = [[] for _ in range(S)]
    for i in by_id[live[by_id]].tolist():
        bins_of[scaf[i]].append(i)
    records = []
    for s, name in enumerate(names):
        d, rows = density[s], bins_of[s]
        rec = {"scaffold": name, "bins": int(scaffoldBins[name]), "live_bins": int(L[s]),
               "assigned": int(np.argmax(own[s])) if own[s].any() else None,
               "best": None, "best_density": None, "second": None, "second_density": None, "ratio": None,
               "density": d.tolist(), "live_ids": [int(ids[i]) for i in rows]}
        if L[s] == 0 or not d.any():
            rec["verdict"] = "no_contacts"
        else:
            best = int(np.argmax(d))                       # numpy.argmax: the lowest index among equals
            rec["best"], rec["best_density"], rec["ratio"] = best, float(d[best]), float("inf")
            if G > 1:
                rest = d.copy()
                rest[best] = -np.inf
                second = int(np.argmax(rest))
                rec["second"], rec["second_density"] = second, float(d[second])
                if d[second] != 0.0:
                    rec["ratio"] = float(d[best] / d[second])
            if rec["assigned"] is not None:
                rec["verdict"] = "supported" if best == rec["assigned"] else "contested"
            else:
                rec["verdict"] = "rescued" if rec["ratio"] >= minRatio else "ambiguous"
        if rows:
            denom = (m - own[s])[None, :]
            v = np.divide(binsum[rows], denom, out=np.zeros((len(rows), G)), where=denom != 0)
            side = [str(a + 1) if hit else "-" for a, hit in zip(v.argmax(axis=1).tolist(), v.any(axis=1).tolist())]
        else:
            side = []
        rec["runs"] = _run_lengths(side)
        records.append(rec)
    return records


def _gs_text(v):
    return "NA" if v is None else (repr(v) if isinstance(v, float) else str(v))


def _gs_group(g):
    return None if g is None else g + 1


def groupSupportText(records):
    """The report: a '#' header line, then one tab-separated line per scaffold in bed order.  Groups are the file's
    1-based numbers, floats are written with repr, a missing value is NA."""
    text = ["#scaffold\tbins\tlive_bins\tassigned\tbest\tbest_density\tsecond\tsecond_density\tratio\tverdict\truns\n"]
    for r in records:
        text.append("\t".join([r["scaffold"], str(r["bins"]), str(r["live_bins"]), _gs_text(_gs_group(r["assigned"])),
                               _gs_text(_gs_group(r["best"])), _gs_text(r["best_density"]), _gs_text(_gs_group(r["second"])),
                               _gs_text(r["second_density"]), _gs_text(r["ratio"]), r["verdict"], r["runs"]]) + "\n")
    return "".join(text)


def writeGroupSupportToFile(records, outFile, fullDir=None):
    """groupSupportText to ``outFile``; ``fullDir``: also the S x G density table as ``groupSupport.full.tsv``."""
    _write_text(outFile, groupSupportText(records))
    if fullDir:
        os.makedirs(fullDir, exist_ok=True)
        G = len(records[0]["density"]) if records else 0
        with open(os.path.join(fullDir, "groupSupport.full.tsv"), "w") as fh:
            fh.write("\t".join(["scaffold"] + ["group%d" % (g + 1) for g in range(G)]) + "\n")
            for r in records:
                fh.write("\t".join([r["scaffold"]] + [repr(float(v)) for v in r["density"]]) + "\n")
    print("Group support written for scaffolds " + str(len(records)))


def writeRescuedGroupsToFile(records, chromosomeGroupFile, outFile):
    """``chromosomeGroupFile`` again - its groups in its order and numbering, every line verbatim - with, after each
    group's own lines, the present non-zero-row bins of the scaffolds rescued into it as ``binID<TAB>scaffold`` (scaffolds
    in bed order, bins ascending).  One pass: the rescued scaffolds were scored against the input's groups only.
    Returns the number of rescued scaffolds."""
    with open(chromosomeGroupFile) as fh:
        lines = fh.read().splitlines(keepends=True)
    groups = []                                            # the first line is group 1's header (orderGenome.readChromsFromFile)
    for k, line in enumerate(lines):
        if k == 0 or line[0] == "#":
            groups.append([line])
        else:
            groups[-1].append(line)
    rescued = [r for r in records if r["verdict"] == "rescued"]
    text = []
    for g, group in enumerate(groups):
        if not group[-1].endswith("\n"):
            group[-1] += "\n"
        text.extend(group)
        for r in rescued:
            if r["best"] == g:
                text.extend(str(b) + "\t" + r["scaffold"] + "\n" for b in r["live_ids"])
    _write_text(outFile, "".join(text))
    print("Scaffolds rescued into chromosome groups " + str(len(rescued)))
    return len(rescued)


def groupSupportToFiles(matrix, binList, chromList, hicProBedFile, chromosomeGroupFile, groupSupportFile=None,
                        rescuedChromosomeGroupFile=None, minRatio=3.0, fullDir=None):
    """groupSupport of a resident map and the files wanted of it; returns the records."""
    records = groupSupport(matrix, binList, chromList, readScaffoldBinCounts(hicProBedFile), minRatio=minRatio)
    if groupSupportFile:
        writeGroupSupportToFile(records, groupSupportFile, fullDir)
    if rescuedChromosomeGroupFile:
        writeRescuedGroupsToFile(records, chromosomeGroupFile, rescuedChromosomeGroupFile)
    return records


# ------------------------------------------------------------------------------------------------
def runPipeline(hicProBedFile, hicProBiasFile, hicProMatrixFile, hicProScaffSizeFile,
                dendrogramOrderFile, avgClusterPlot, avgClusterPlot_outlined,
                binGroupFile, assessmentFile, chromosomeGroupFile,
                hyperGeom, hmm, minSize, modularity, louvainRounds,
                psig, convergenceRounds, lookAhead, resolution, device=0, shard=None, keep_resident=False,
                groupSupportFile=None, rescuedChromosomeGroupFile=None, contacts_ctx=None):
    """S2C:1104-1174, same positional arguments (``device``, ``shard``, ``keep_resident`` and the two file names are
    optional extras; ``groupSupportFile`` / ``rescuedChromosomeGroupFile``: also write the group-support report and the
    group file with the rescued scaffolds (groupSupport) from the resident map;
    ``shard=(rank, world)``: this process is one of ``world`` that work on the same map, see runResident;
    ``keep_resident=True``: the context with the contact matrix in HBM is not closed but returned as
    ``(DeviceMatrix, bins of its rows)`` so that Part 2 of the same run need not parse the text matrix again;
    ``contacts_ctx``: a context that already holds the matrix of exactly the bins the two files give - ``-part0`` of the
    same run (iceNormalize.runPipeline(..., keep_resident=True)) - used in place of the text parse; it is closed like
    a context made here)."""
    print("########################################")
    print("### Working on Part1 of the pipeline ###")
    t_all = time.time()
    use_hmm = hyperGeom is not True and hmm is True and hmm_enabled()
    if hyperGeom is not True and not use_hmm:
        raise NotImplementedError("only the hyperGeom = True strategy is implemented on MI355X by default; hmm = True "
                                  "(hmmlearn's EM, restated with a seeded initialisation) needs HICMI_HMM=1")
    binList = initiateLoci(hicProBedFile, hicProBiasFile)
    if contacts_ctx is not None:
        if contacts_ctx.n != len(binList):
            contacts_ctx.close()
            raise ValueError("the resident matrix has %d rows, the bed and biases files give %d bins" % (contacts_ctx.n, len(binList)))
        print("Rows in adjacency matrix " + str(len(binList)))
        adjMat = DeviceMatrix(contacts_ctx)
    else:
        adjMat = buildAdjacencyMatrix(hicProMatrixFile, binList, device=device)
    try:
        cutIndices = runResident(adjMat, binList, hicProScaffSizeFile, dendrogramOrderFile, binGroupFile,
                                 assessmentFile, chromosomeGroupFile, minSize, modularity, psig,
                                 louvainRounds=louvainRounds, shard=shard, hmm=use_hmm,
                                 convergenceRounds=convergenceRounds, lookAhead=lookAhead)
        # S2C:1124 / S2C:1155-1156: the clustered distance matrix, then - groups outlined - the distance transform of
        # the un-logged similarity matrix, which is the distance matrix again up to a few roundings
        if plotModule.plots_enabled(avgClusterPlot):
            plotModule.plotContactMap(plotModule.DeviceImage(adjMat.ctx, 1, adjMat.order), resolution=resolution,
                                      highlightChroms=False, showPlot=False, savePlot=avgClusterPlot)
        if plotModule.plots_enabled(avgClusterPlot_outlined):
            plotModule.plotContactMap(plotModule.DeviceImage(adjMat.ctx, 1, adjMat.order), resolution=resolution,
                                      highlightChroms=cutIndices, showPlot=False, savePlot=avgClusterPlot_outlined)
        if groupSupportFile or rescuedChromosomeGroupFile:
            groupSupportToFiles(adjMat, adjMat.kept_bins, adjMat.chromosome_groups, hicProBedFile, chromosomeGroupFile,
                                groupSupportFile, rescuedChromosomeGroupFile)
    except BaseException:
        adjMat.ctx.close()
        raise
    if not keep_resident:
        adjMat.ctx.close()
    print("Total run-time of Part1 = " + str(time.time() - t_all))
    print("CutIndices = " + str(cutIndices))
    print("- Part 1 (grouping bins to groups) completed successfully")
    return (adjMat, adjMat.kept_bins) if keep_resident else None


class _FileWriter:
    """Part 1's text files written on one background thread while the device keeps working: the strings are built and
    written in submission order; ``finish()`` returns when every file is on disk and re-raises what a writer raised.
    Jobs submitted with ``deferred=True`` wait for ``release()``: formatting 16,000 lines holds the interpreter lock, so
    the caller releases them when it enters a long native call (Part 2's lock-step insertion), not while its own
    Python threads are busy."""

    def __init__(self, enabled):
        import threading
        from concurrent.futures import ThreadPoolExecutor
        self.pool = ThreadPoolExecutor(max_workers=1) if enabled else None
        self.gate = threading.Event()
        self.jobs = []

    def submit(self, fn, *args, deferred=False):
        if self.pool is None:
            return fn(*args)
        if deferred:
            def held(*a):
                self.gate.wait()
                return fn(*a)
            self.jobs.append(self.pool.submit(held, *args))
        else:
            self.jobs.append(self.pool.submit(fn, *args))

    def release(self):
        self.gate.set()

    def finish(self):
        self.gate.set()
        for j in self.jobs:
            j.result()
        self.jobs = []
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None


def _cluster_resident(adjMat: DeviceMatrix, binList, hicProScaffSizeFile, mark, t0):
    """runResident's stages from removeRows to the similarity stage in leaf order (S2C:1117-1131): returns
    (adjMat, binList in leaf order, dendrogram, prep) - ``prep`` holds the host tables built beside the chain."""
    adjMat, binList = removeRows(adjMat, binList, zeroRows=True, biasVals=False, store_row_sums=False)
    adjMat.kept_bins = list(binList)                  # rows of the device matrix, in .bed order
    adjMat = convertMatrix(adjMat, binList, distance=True, similarity=False)
    mark("row sums")
    # host work that does not depend on the tree runs while the chain does (a single ~100 ms native call): the labels,
    # the size table and the scaffold -> bins table of the assessment
    prep = {}

    def meanwhile(bl=binList, sums=adjMat.seq_sum):
        _store_row_sums(bl, sums)                     # (Bin.rowSum, S2C:133-135: nothing reads it before the chain ends)
        prep["labels"] = [b.chrom + '_' + str(b.ID) for b in bl]
        prep["sizes"] = readSizeFileToDict(hicProScaffSizeFile)
        prep["scaffolds"] = _scaffold_bins((b.ID, b.chrom) for b in bl)
        prep["pairs"] = _bin_pairs(bl)
        # the text of the three per-bin files, line by line: ~12 ms of formatting at 16k that would otherwise hold the
        # interpreter lock while Part 2's threads want it (the writer thread only joins the lines)
        prep["dend_lines"] = [lab + "\t" + str(i) for i, lab in enumerate(prep["labels"])]
        prep["bin_lines"] = {b.ID: _bin_line(b) for b in bl}
        prep["entry_lines"] = {int(b.ID): str(int(b.ID)) + "\t" + str(b.chrom) + "\n" for b in bl}
    # ('ivl', the labels in leaf order, is only wanted by the dendrogram file, whose lines are ready: prep["dend_lines"])
    dendrogram = averageClusterNodes(adjMat, lambda: prep["labels"], noPlot=True, meanwhile=meanwhile, want_ivl=False)
    mark("UPGMA + leaf order")
    # the reference parses the file back (readDengrogramLeavesFromFile); the leaves are the same integers
    adjMat, binList = reorderMatrix(adjMat, binList, dendrogram['leaves'])
    print("Total run-time to cluster = " + str(time.time() - t0))
    adjMat = convertMatrix(adjMat, binList, distance=False, similarity=True)
    return adjMat, binList, dendrogram, prep


def runResident(adjMat: DeviceMatrix, binList, hicProScaffSizeFile, dendrogramOrderFile, binGroupFile,
                assessmentFile, chromosomeGroupFile, minSize, modularity, psig, louvainRounds=20, shard=None,
                overlap_files=False, hmm=False, convergenceRounds=5, lookAhead=.2):
    """S2C:1117-1167 on a contact map that is already resident in HBM (what bench.py times): every
    stage after the text loaders, including the small intermediate files the reference round-trips
    through.  Returns the filtered cut indices; ``binList`` is left in .bed order for the caller.

    ``overlap_files=True``: the four files are written by a background thread (the dendrogram order while the rows
    are sorted and scanned, the three group files while the caller goes on); the caller hands
    ``adjMat.chromosome_groups`` - what Part 2 would read back from chromosomeGroupFile - to
    ``orderGenome.runResident(..., chromosomeList=, on_native_phase=adjMat.release_files)`` and calls
    ``adjMat.finish_files()`` before it uses the files.

    ``hmm=True``: the boundaries come from identifyChromosomeGroupsHMM (S2C:1138-1140, with ``convergenceRounds`` and
    ``lookAhead``) instead of the rank matrix and the two hypergeometric scans; everything after is the same."""
    writer = _FileWriter(overlap_files)
    adjMat.finish_files = writer.finish
    adjMat.release_files = writer.release
    marks = [("start", time.perf_counter())] if os.environ.get("HICMI_STEP_PROFILE") else None

    def mark(name):
        if marks is not None:
            marks.append((name, time.perf_counter()))
    with paused_gc():
        t0 = time.time()
        if shard is not None:
            # ONE map over shard[1] ranks: the row sums, the row sort / rank matrix and the per-row counts of
            # the scans are computed for rows == shard[0] (mod shard[1]) only and all-gathered; UPGMA and the host control
            # flow run on every rank (deterministic: all ranks write the same files)
            adjMat.ctx.set_row_shard(shard[0], shard[1])
        adjMat, binList, dendrogram, prep = _cluster_resident(adjMat, binList, hicProScaffSizeFile, mark, t0)
        t0 = time.time()
        if hmm:
            # S2C:1138-1140: every rank of a shard runs the HMM whole (the matrix and the gathered row sums are on each)
            writer.submit(dendrogramLeafOrder_toFile, dendrogram, dendrogramOrderFile, prep["dend_lines"])
            mark("reorder")
            adjMat.hmm = HmmDevice(adjMat)
            cutIndices = identifyChromosomeGroupsHMM(adjMat, binList, minSize=minSize, modularity=modularity,
                                                     convergenceRounds=convergenceRounds, lookAhead=lookAhead,
                                                     louvainRounds=louvainRounds)
            if adjMat.hmm.profile:
                adjMat.hmm.report()
            mark("HMM boundaries")
        else:
            argsorted_adjMat = rankOrderMatrix(adjMat)
            # the dendrogram file (16k formatted lines: ~5 ms of interpreter time) is handed to the writer thread only
            # now: the two scan loops that follow are native calls that release the interpreter lock, the list work
            # above is not
            writer.submit(dendrogramLeafOrder_toFile, dendrogram, dendrogramOrderFile, prep["dend_lines"])
            mark("reorder + rank matrix")
            initial_cut_inds = pre_process_all_matrix_breakpoints(argsorted_adjMat, min_size=minSize,
                                                                  min_frac=modularity, psig=psig)
            mark("first-pass scans")
            cutIndices = filter_noisy_breakpoints(argsorted_adjMat, initial_cut_inds, psig=psig)
            mark("filter scans")
        if modularity is not False and modularity > 0.0:
            # S2C:1148-1152: Louvain on log10(similarity + 1) of the bins after the last cut index (modularity.py:
            # seeded restatement of python-louvain; level 0 on the device with HICMI_LOUVAIN_DEVICE=1)
            start = sorted(cutIndices)[-1] if len(cutIndices) else 0
            if len(adjMat.order) - start > 0:
                new_order, cutIndices = _louvain_tail(adjMat, binList, cutIndices, louvainRounds)
                adjMat, binList = reorderMatrix(adjMat, binList, new_order)
        writer.submit(writeBinGroupingsToFile, list(cutIndices), list(binList), binGroupFile, prep["bin_lines"], deferred=True)
        binGroups = _bin_group_pairs(cutIndices, binList, prep["pairs"])
        print("Total run-time to identify chromosome boundaries = " + str(time.time() - t0))
        t0 = time.time()
        fastaSizeDict = prep["sizes"]
        print(str(len(binGroups)) + " chromosomes read in from file")      # == readBinGroupingsFromFile(binGroupFile)
        chrGroups = assessChromosomeClustering(binGroups, assessmentFile,
                                               write=lambda fn, *a: writer.submit(fn, *a, deferred=True),
                                               scaffolds=None if (modularity is not False and modularity > 0.0) else prep["scaffolds"])
        adjMat.chromosome_groups = rankChromosomeGroups(chrGroups, fastaSizeDict)
        writer.submit(writeChromosomeGroupingsToFile, chrGroups, fastaSizeDict, chromosomeGroupFile, prep["entry_lines"],
                      deferred=True)
        print("Total run-time to assign scaffolds to chromosomes = " + str(time.time() - t0))
        mark("groups + assessment")
    if not overlap_files:
        writer.finish()
    if marks is not None:
        sys.stderr.write("[hicmi] part1 host timeline (ms): " + ", ".join(
            "%s %.1f" % (b[0], (b[1] - a[1]) * 1e3) for a, b in zip(marks, marks[1:])) + "\n")
    return cutIndices
