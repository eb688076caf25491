"""NumPy restatement of the HMM boundary finder (S2C:730-942, hmm = True) - test infrastructure only.

hmmlearn 0.3's GaussianHMM(n_components=2, covariance_type="diag", n_iter=1000, init_params="cm", params="cmt") and
sklearn's KMeans, restated from their formulas; neither library is needed.  The forward /
backward pass runs in the scaled probability domain (the same quantities as hmmlearn's log-space lattice, to ~1e-13),
which keeps the sequential loop cheap enough for 2,000-bin maps.
"""
from __future__ import annotations

import math

import numpy as np

N_ITER, TOL, MIN_COVAR = 1000, 1e-2, 1e-3
STARTPROB = np.array([.5, .5])
TRANSMAT = np.array([[.9, .1], [.0001, .9999]])


# ---- k-means (sklearn _kmeans_plusplus / _kmeans_single_lloyd, k = 2) --------------------------------------------
def dist2(X, rows):
    return np.vstack([((X - X[r]) ** 2).sum(axis=1) for r in rows])


def _assign(X, centers):
    d0 = ((X - centers[0]) ** 2).sum(axis=1)
    d1 = ((X - centers[1]) ** 2).sum(axis=1)
    labels = (d1 < d0).astype(np.int32)                    # ties to cluster 0
    return labels, np.where(labels == 1, d1, d0)


def kmeans_lloyd(X, centers, max_iter=300, tol=0.0):
    """(centers, labels, inertia, iterations).  An empty cluster keeps its center."""
    X = np.asarray(X, dtype=np.float64)
    centers = np.array(centers, dtype=np.float64)
    labels_old = np.full(len(X), -1, np.int32)
    strict = False
    it = 0
    for it in range(1, max_iter + 1):
        labels, mind = _assign(X, centers)
        new = centers.copy()
        for k in range(2):
            sel = labels == k
            if sel.any():
                new[k] = X[sel].sum(axis=0) / sel.sum()
        shift = float(((new - centers) ** 2).sum())
        centers = new
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if shift <= tol:
            break
        labels_old = labels
    if not strict:
        labels, mind = _assign(X, centers)
    return centers, labels, float(mind.sum()), it


def kmeans_plusplus_rows(X, rng):
    T = len(X)
    first = int(rng.integers(T))
    closest = dist2(X, [first])[0]
    rand_vals = rng.uniform(size=2) * closest.sum()
    cand = np.minimum(np.searchsorted(np.cumsum(closest), rand_vals), T - 1)
    dist = np.minimum(closest, dist2(X, cand))
    return [first, int(cand[int(np.argmin(dist.sum(axis=1)))])]


def init_params(X, seed, fit_index, restarts=10):
    """(means, covars, k-means iterations): best of ``restarts`` seeded k-means++ / Lloyd runs; diag cov + min_covar."""
    T = len(X)
    var0 = X.var(axis=0)
    tol = 1e-4 * float(np.mean(var0))
    best, iters = None, 0
    for r in range(restarts):
        rng = np.random.default_rng([seed, fit_index, r])
        rows = kmeans_plusplus_rows(X, rng)
        centers, _lab, inertia, it = kmeans_lloyd(X, X[rows], 300, tol)
        iters += it
        if best is None or inertia < best[1]:
            best = (centers, inertia)
    var1 = ((X - X.mean(axis=0)) ** 2).sum(axis=0) / (T - 1)
    return best[0], np.vstack([var1 + MIN_COVAR, var1 + MIN_COVAR]), iters


# ---- the HMM -----------------------------------------------------------------------------------------------------
def emission(X, means, covars):
    """log N(x_t; mu_k, diag(var_k)), T x 2 (hmmlearn log_multivariate_normal_density_diag)."""
    D = X.shape[1]
    return -0.5 * (D * np.log(2 * np.pi) + np.sum(np.log(covars), 1) + np.sum((means ** 2) / covars, 1)
                   - 2 * np.dot(X, (means / covars).T) + np.dot(X ** 2, (1.0 / covars).T))


def estep(L, startprob, transmat):
    """(logprob, gamma T x 2, xi 2 x 2) - forward / backward in the scaled domain."""
    T = len(L)
    m = L.max(axis=1)
    E = np.exp(L - m[:, None])
    A = [[float(v) for v in row] for row in transmat]
    e0, e1 = E[:, 0].tolist(), E[:, 1].tolist()
    al = np.empty((T, 2))
    sc = np.empty(T)
    a0, a1 = startprob[0] * e0[0], startprob[1] * e1[0]
    s = a0 + a1
    a0, a1 = a0 / s, a1 / s
    al[0] = a0, a1
    sc[0] = s
    for t in range(1, T):
        n0 = (a0 * A[0][0] + a1 * A[1][0]) * e0[t]
        n1 = (a0 * A[0][1] + a1 * A[1][1]) * e1[t]
        s = n0 + n1
        a0, a1 = n0 / s, n1 / s
        al[t] = a0, a1
        sc[t] = s
    logprob = float(np.log(sc).sum() + m.sum())
    be = np.empty((T, 2))
    b0, b1 = 1.0, 1.0
    be[T - 1] = b0, b1
    for t in range(T - 2, -1, -1):
        w0, w1 = e0[t + 1] * b0, e1[t + 1] * b1
        s = sc[t + 1]
        b0, b1 = (A[0][0] * w0 + A[0][1] * w1) / s, (A[1][0] * w0 + A[1][1] * w1) / s
        be[t] = b0, b1
    g = al * be
    g /= g.sum(axis=1, keepdims=True)
    xi = np.zeros((2, 2))
    if T > 1:
        w = E[1:] * be[1:] / sc[1:, None]
        xi = np.asarray(A) * (al[:-1].T @ w)
    return logprob, g, xi


def mstep(X, g, xi, means, covars, transmat):
    post = g.sum(axis=0)
    obs = g.T @ X
    obs2 = g.T @ (X ** 2)
    denom = post[:, None]
    means = obs / denom
    covars = (1e-2 + (obs2 - 2 * means * obs + means ** 2 * denom)) / np.maximum(denom, 1e-5)
    t = np.where(transmat == 0, 0, np.maximum(xi, 0))
    rs = t.sum(axis=1, keepdims=True)
    rs[rs == 0] = 1
    return means, covars, t / rs


def fit(X, means, covars, transmat, startprob=STARTPROB, n_iter=N_ITER, tol=TOL):
    """Baum-Welch as hmmlearn's BaseHMM.fit: (means, covars, transmat, logprob history)."""
    X = np.asarray(X, dtype=np.float64)
    means, covars, transmat = np.array(means, float), np.array(covars, float), np.array(transmat, float)
    hist = []
    for _ in range(n_iter):
        lp, g, xi = estep(emission(X, means, covars), startprob, transmat)
        means, covars, transmat = mstep(X, g, xi, means, covars, transmat)
        hist.append(lp)
        if len(hist) >= 2 and hist[-1] - hist[-2] < tol:
            break
    return means, covars, transmat, np.array(hist)


def viterbi(X, means, covars, transmat, startprob=STARTPROB):
    L = emission(np.asarray(X, dtype=np.float64), means, covars)
    T = len(L)
    with np.errstate(divide="ignore"):
        lA = np.log(transmat).tolist()
        lp = np.log(startprob).tolist()
    l0, l1 = L[:, 0].tolist(), L[:, 1].tolist()
    d = np.empty((T, 2))
    d0, d1 = lp[0] + l0[0], lp[1] + l1[0]
    d[0] = d0, d1
    for t in range(1, T):
        d0, d1 = max(d0 + lA[0][0], d1 + lA[1][0]) + l0[t], max(d0 + lA[0][1], d1 + lA[1][1]) + l1[t]
        d[t] = d0, d1
    states = np.zeros(T, np.int32)
    states[T - 1] = 1 if d[T - 1, 1] > d[T - 1, 0] else 0
    for t in range(T - 2, -1, -1):
        j = states[t + 1]
        states[t] = 1 if d[t, 1] + lA[1][j] > d[t, 0] + lA[0][j] else 0
    return states


class NumpyBackend:
    """``hmm_states(c, p)`` on a host matrix (log10(similarity + 1) in the current order), seeded as the device path."""

    def __init__(self, logsim, seed=0):
        self.A = np.asarray(logsim, dtype=np.float64)
        self.seed = seed
        self.fit_index = 0
        self.log = []

    def __len__(self):
        return len(self.A)

    def hmm_states(self, c, p):
        X = self.A[c:, c:p]
        means, covars, _ = init_params(X, self.seed, self.fit_index)
        means, covars, transmat, hist = fit(X, means, covars, TRANSMAT)
        self.fit_index += 1
        self.log.append((c, p, len(hist)))
        return viterbi(X, means, covars, transmat)


# ---- the control flow, literally (S2C:730-942) ------------------------------------------------------------------
def identifyBoundry(hiddenStates, cutIndices, switchCount=10):
    countDict = {0: 0, 1: 0}
    for s in hiddenStates[0:switchCount]:
        countDict[int(s)] += 1
    startState = sorted([[s, c] for s, c in countDict.items()], key=lambda x: x[1], reverse=True)[0][0]
    states = [hiddenStates[ind:ind + switchCount] for ind in range(0, len(hiddenStates) - switchCount)]
    cutInd = 0
    for ind, s in enumerate(states):
        if sum([1 for hS in s if hS != startState]) == switchCount:
            cutInd = ind + cutIndices[-1]
            break
    return cutInd


def hmmChromosomes(backend, cutIndices, minSize=20, convergenceRounds=8, lookAhead=False):
    n = len(backend)
    if lookAhead != False:  # noqa: E712
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
        width = len(range(c, min(prevCutInd, n)))
        if width < minSize:
            cutInd = lookAhead
        else:
            cutInd = identifyBoundry(list(backend.hmm_states(c, c + width)), cutIndices, switchCount=minSize)
        if cutInd != prevCutInd:
            prevCutInd = cutInd
            roundCount += 1
            continue
        cutIndices.append(int(cutInd))
        break
    if roundCount > convergenceRounds:
        cutIndices.append(int(cutInd))
    return cutIndices


def identifyChromosomeGroupsHMM(backend, minSize=5, modularity=.05, convergenceRounds=5, lookAhead=.2, prev_cutInds=False):
    """The reference's IndexError at S2C:920 (no cut left) becomes [] here, as in the product."""
    n = len(backend)
    remainder = float(n) - (modularity * float(n))
    cutIndices = [0]
    if modularity == 1:
        return []
    if prev_cutInds is not False:
        cutIndices = prev_cutInds
    while cutIndices[-1] <= remainder:
        cutIndices = hmmChromosomes(backend, cutIndices, minSize, convergenceRounds, lookAhead)
        if cutIndices[-1] == 0:
            break
        if cutIndices[-1] == "NA":
            cutIndices.pop(-1)
            break
    if cutIndices[0] == 0:
        cutIndices.pop(0)
    if not cutIndices:
        return []
    if cutIndices[-1] == n:
        cutIndices.pop(-1)
        if not cutIndices:
            return []
        if (n - cutIndices[-1]) >= (5 * (n * modularity)):
            if convergenceRounds - 1 == 0:
                return cutIndices
            cutIndices = identifyChromosomeGroupsHMM(backend, 5, .05, convergenceRounds - 1, .5, prev_cutInds=cutIndices)
    return cutIndices


def log_similarity(contacts, order):
    """log10(similarity + 1) (0 where similarity == 0) of a contact matrix in ``order`` (S2C:147-149, 165-183), with
    the row sums of the reference (numpy sum, builtin sum)."""
    C = np.asarray(contacts, dtype=np.float64)
    np_sum = C.sum(axis=1)
    seq_sum = np.array([sum(row) for row in C.tolist()])
    d = (1.0 - (C / np_sum[:, None])) + 1.0
    s = seq_sum[:, None] * (1.0 - (d - 1.0))
    s = s[np.ix_(order, order)]
    out = np.zeros_like(s)
    nz = s != 0.0
    out[nz] = np.log(s[nz] + 1.0) / math.log(10)
    return out
