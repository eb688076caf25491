"""Exact references for the 2-state HMM kernels (k_hmm.hip) - test infrastructure only, NumPy and mpmath.

Two independent statements of the same operations, neither of which shares code with hmm_reference.py:
  * ``brute_force``: the definition itself, a sum (or a maximum) over all 2^T state paths in mpmath;
  * serial log-space forward / backward / Viterbi, the emission, one M-step and the column statistics in
    numpy.longdouble (64-bit mantissa on x86), with -inf handled explicitly.
The longdouble recursions are held to ``brute_force`` in test_hmm_exact_cpu.py; the device kernels and the fp64
restatement in hmm_reference.py are held to the longdouble recursions.

The second half of the file builds the inputs of the step tests (test_gpu_hmm_steps.py), so that the CPU suite can assert
the conditions those tests rely on (unsaturated posteriors, Viterbi margins) on exactly the same arrays.

The third part does the same for what runs before the EM (test_gpu_kmeans_steps.py): squared distances, Lloyd's
iteration with sklearn's stop rules, the seeded k-means++ choice and the log-similarity observations in longdouble;
Lloyd's iteration once more in Python ints and fractions.Fraction, for integer data on which fp64 cannot round; and the
inputs of those tests.
"""
from __future__ import annotations

import functools
import itertools
from fractions import Fraction
from types import SimpleNamespace

import mpmath
import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS_LD = float(np.finfo(LD).eps)
NINF = LD(-np.inf)
PI_LD = LD("3.14159265358979323846264338327950288")
MIN_COVAR = 1e-3
SCAN_THREADS = 512                                         # kScanThreads of k_hmm.hip


# ---- the definition: all 2^T paths --------------------------------------------------------------------------------
def brute_force(L, startprob, transmat, dps=60):
    """(logprob, gamma T x 2, xi 2 x 2, set of maximum-score paths, their score) from the 2^T paths, in mpmath at ``dps``
    digits.

    weight(s) = pi[s_0] e^{L_0[s_0]} prod_{t >= 1} A[s_{t-1}][s_t] e^{L_t[s_t]}; logprob = log sum_s weight(s);
    gamma_t[k] = sum_{s: s_t = k} weight / total; xi[i][j] = sum_t sum_{s: s_t = i, s_{t+1} = j} weight / total.
    Everything is returned as mpmath numbers; the optimal paths as tuples."""
    L = np.asarray(L, dtype=np.float64)
    T = len(L)
    assert 1 <= T <= 10 and dps >= 50
    with mpmath.workdps(dps):
        mp = mpmath.mpf
        first = [mp(float(startprob[k])) * mpmath.exp(mp(float(L[0, k]))) for k in range(2)]
        step = [[[mp(float(transmat[i][j])) * mpmath.exp(mp(float(L[t, j]))) for j in range(2)] for i in range(2)]
                for t in range(T)]
        total = mp(0)
        gamma = [[mp(0), mp(0)] for _ in range(T)]
        xi = [[mp(0), mp(0)], [mp(0), mp(0)]]
        weights = {}
        for s in itertools.product((0, 1), repeat=T):
            w = first[s[0]]
            for t in range(1, T):
                w = w * step[t][s[t - 1]][s[t]]
            weights[s] = w
            total += w
            for t in range(T):
                gamma[t][s[t]] += w
            for t in range(T - 1):
                xi[s[t]][s[t + 1]] += w
        assert total > 0, "no path has positive probability"
        gamma = [[g / total for g in row] for row in gamma]
        xi = [[v / total for v in row] for row in xi]
        wmax = max(weights.values())
        slack = mp(10) ** (-(dps - 10))
        best = {s for s, w in weights.items() if w >= wmax * (1 - slack)}
        return mpmath.log(total), gamma, xi, best, mpmath.log(wmax)


def to_ld(v):
    """An mpmath number as a longdouble (through 30 significant digits)."""
    return LD(mpmath.nstr(v, 30))


# ---- longdouble, serial ---------------------------------------------------------------------------------------------
def _log(p):
    """log of probabilities in longdouble, log 0 = -inf."""
    p = np.asarray(p, dtype=np.float64).astype(LD)
    out = np.full(p.shape, NINF, dtype=LD)
    np.log(p, out=out, where=p > 0)
    return out


def _lse(a, b):
    """log(e^a + e^b); -inf is the empty sum."""
    if a < b:
        a, b = b, a
    if b == NINF:
        return a
    return a + np.log1p(np.exp(b - a))


def estep_ld(L, startprob, transmat):
    """Serial forward / backward in log space: alpha, beta, gamma (T x 2), xi (2 x 2), logprob - all longdouble.

    alpha_0[j] = log pi[j] + L_0[j];  alpha_t[j] = logsumexp_i(alpha_{t-1}[i] + log A[i][j]) + L_t[j];
    beta_{T-1} = 0;  beta_t[i] = logsumexp_j(log A[i][j] + L_{t+1}[j] + beta_{t+1}[j]);
    gamma_t = exp(alpha_t + beta_t - logprob);  xi[i][j] = sum_t exp(alpha_t[i] + log A[i][j] + L_{t+1}[j] +
    beta_{t+1}[j] - logprob)."""
    L = np.asarray(L).astype(LD)
    T = len(L)
    lpi, lA = _log(startprob), _log(transmat)
    a00, a01, a10, a11 = lA[0, 0], lA[0, 1], lA[1, 0], lA[1, 1]
    alpha = np.empty((T, 2), dtype=LD)
    beta = np.empty((T, 2), dtype=LD)
    p0, p1 = lpi[0] + L[0, 0], lpi[1] + L[0, 1]
    alpha[0] = p0, p1
    for t in range(1, T):
        p0, p1 = _lse(p0 + a00, p1 + a10) + L[t, 0], _lse(p0 + a01, p1 + a11) + L[t, 1]
        alpha[t] = p0, p1
    logprob = _lse(p0, p1)
    assert np.isfinite(logprob), "the observations have probability zero under the model"
    b0, b1 = LD(0), LD(0)
    beta[T - 1] = b0, b1
    for t in range(T - 2, -1, -1):
        w0, w1 = L[t + 1, 0] + b0, L[t + 1, 1] + b1
        b0, b1 = _lse(a00 + w0, a01 + w1), _lse(a10 + w0, a11 + w1)
        beta[t] = b0, b1
    gamma = np.exp(alpha + beta - logprob)
    xi = np.zeros((2, 2), dtype=LD)
    if T > 1:
        w = L[1:] + beta[1:]                                # (T-1) x 2, indexed by the target state
        for i in range(2):
            for j in range(2):
                xi[i, j] = np.exp(alpha[:-1, i] + lA[i, j] + w[:, j] - logprob).sum()
    finite = alpha[np.isfinite(alpha)]
    return SimpleNamespace(alpha=alpha, beta=beta, gamma=gamma, xi=xi, logprob=logprob,
                           max_alpha=float(np.abs(finite).max()))


def _margin(x, y):
    """|x - y|; two impossible alternatives (-inf, -inf) compare equal in any arithmetic, so the tie rule decides them
    identically everywhere: that comparison cannot be lost to rounding and its margin is reported as +inf."""
    if x == NINF and y == NINF:
        return LD(np.inf)
    return abs(x - y)


def viterbi_ld(L, startprob, transmat):
    """Serial Viterbi in longdouble, ties to state 0 in the last state and in every back-pointer.

    Returns delta (T x 2), states, the back-pointer margins |(delta_t[1] + log A[1][j]) - (delta_t[0] + log A[0][j])|
    ((T - 1) x 2) and the final-state margin |delta_{T-1}[1] - delta_{T-1}[0]|."""
    L = np.asarray(L).astype(LD)
    T = len(L)
    lpi, lA = _log(startprob), _log(transmat)
    delta = np.empty((T, 2), dtype=LD)
    back = np.zeros((max(T - 1, 0), 2), dtype=np.int8)
    margin = np.empty((max(T - 1, 0), 2), dtype=LD)
    d0, d1 = lpi[0] + L[0, 0], lpi[1] + L[0, 1]
    delta[0] = d0, d1
    for t in range(1, T):
        c = [(d0 + lA[0, 0], d1 + lA[1, 0]), (d0 + lA[0, 1], d1 + lA[1, 1])]
        for j in range(2):
            back[t - 1, j] = 1 if c[j][1] > c[j][0] else 0
            margin[t - 1, j] = _margin(c[j][1], c[j][0])
        d0, d1 = max(c[0]) + L[t, 0], max(c[1]) + L[t, 1]
        delta[t] = d0, d1
    states = np.zeros(T, dtype=np.int32)
    states[T - 1] = 1 if d1 > d0 else 0
    for t in range(T - 2, -1, -1):
        states[t] = back[t, states[t + 1]]
    finite = delta[np.isfinite(delta)]
    return SimpleNamespace(delta=delta, states=states, margin=margin, final_margin=_margin(d1, d0),
                           best=max(d0, d1), max_delta=float(np.abs(finite).max()))


def path_score(L, startprob, transmat, states):
    """log pi[s_0] + L_0[s_0] + sum_t (log A[s_{t-1}][s_t] + L_t[s_t]) in longdouble."""
    L = np.asarray(L).astype(LD)
    lpi, lA = _log(startprob), _log(transmat)
    s = np.asarray(states, dtype=np.int64)
    score = lpi[s[0]] + L[0, s[0]]
    for t in range(1, len(s)):
        score = score + (lA[s[t - 1], s[t]] + L[t, s[t]])
    return score


def emission_ld(X, means, covars):
    """(L, Sabs), both T x 2 longdouble.  L_t[k] = -0.5 (const_k - 2 x_t.(mu_k / v_k) + x_t^2.(1 / v_k)) with
    const_k = D log 2 pi + sum log v_k + sum mu_k^2 / v_k (hmmlearn's log_multivariate_normal_density_diag);
    Sabs_t[k] = |const_k| + 2 sum |x mu / v| + sum x^2 / v, the magnitude the three terms are summed at."""
    X = np.asarray(X, dtype=np.float64).astype(LD)
    mu = np.asarray(means, dtype=np.float64).astype(LD)
    v = np.asarray(covars, dtype=np.float64).astype(LD)
    D = X.shape[1]
    const = D * np.log(2 * PI_LD) + np.log(v).sum(axis=1) + (mu * mu / v).sum(axis=1)
    L = np.empty((len(X), 2), dtype=LD)
    S = np.empty((len(X), 2), dtype=LD)
    for k in range(2):
        cross = X * (mu[k] / v[k])
        quad = X * X / v[k]
        L[:, k] = -0.5 * (const[k] - 2 * cross.sum(axis=1) + quad.sum(axis=1))
        S[:, k] = abs(const[k]) + 2 * np.abs(cross).sum(axis=1) + quad.sum(axis=1)
    return L, S


def em_step_ld(X, gamma, xi, transmat):
    """One M-step in longdouble from gamma and xi, by the rules of k_hmm_mstep_cols / k_hmm_mstep_final (hmmlearn's
    GaussianHMM._do_mstep, diag, covars_prior 1e-2, covars_weight 1):
        post_k = sum_t gamma_t[k];  mu_k = gamma_k^T X / post_k;
        var_k = (1e-2 + gamma_k^T X^2 - 2 mu_k gamma_k^T X + mu_k^2 post_k) / max(post_k, 1e-5);
        A = normalize_rows(where(A == 0, 0, xi)), a row that sums to zero left as it is.
    Also returns the magnitudes the sums are formed at (the conditioning of each output): ``means_scale`` =
    gamma_k^T |X| / post_k and ``covars_scale`` = (1e-2 + gamma^T X^2 + 2 |mu gamma^T X| + mu^2 post) / max(post, 1e-5).
    A state with post_k = 0 gives NaN means and covars, as on the device."""
    X = np.asarray(X, dtype=np.float64).astype(LD)
    g = np.asarray(gamma).astype(LD)
    post = g.sum(axis=0)[:, None]
    obs, obs_abs, obs2 = g.T @ X, g.T @ np.abs(X), g.T @ (X * X)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = obs / post
        floor = np.maximum(post, LD(1e-5))
        var = (LD(1e-2) + (obs2 - 2 * mu * obs + mu * mu * post)) / floor
        mu_scale = obs_abs / post
        var_scale = (LD(1e-2) + (obs2 + 2 * np.abs(mu * obs) + mu * mu * post)) / floor
    A0 = np.asarray(transmat, dtype=np.float64)
    a = np.where(A0 == 0, LD(0), np.maximum(np.asarray(xi).astype(LD), LD(0)))
    rs = a.sum(axis=1, keepdims=True)
    rs[rs == 0] = 1
    return SimpleNamespace(means=mu, covars=var, transmat=a / rs, means_scale=mu_scale, covars_scale=var_scale,
                           post=post[:, 0])


def col_stats_ld(X):
    """(column means, column sums of squared deviations from them) in longdouble."""
    X = np.asarray(X, dtype=np.float64).astype(LD)
    mean = X.sum(axis=0) / len(X)
    dev = X - mean
    return mean, (dev * dev).sum(axis=0)


# ---- the inputs of the step tests ---------------------------------------------------------------------------------
SYM = np.array([[.9, .1], [.1, .9]])
REF = np.array([[.9, .1], [.0001, .9999]])                 # hmm_reference.TRANSMAT
HALF = np.array([.5, .5])
ABSORB0 = np.array([[1., 0.], [.5, .5]])
ABSORB1 = np.array([[.5, .5], [0., 1.]])


def chunk_steps(T):
    """S of k_hmm_fb / k_hmm_viterbi: thread k owns steps [min(T, k S), min(T, k S + S))."""
    return (T + SCAN_THREADS - 1) // SCAN_THREADS


def edge_lengths():
    """Two lengths from the kernels' chunk formula, the smallest above 1025 with S >= 2 of each kind: one where
    k S == T for a k < 511 (thread k and all after it own nothing, thread k - 1 a full chunk), and one where the last
    active thread owns exactly one step."""
    full = next(T for T in range(1026, 4096) if T % chunk_steps(T) == 0 and T // chunk_steps(T) < SCAN_THREADS - 1)
    one = next(T for T in range(1026, 4096) if T % chunk_steps(T) == 1)
    return full, one


T_GRID = (1, 2, 3, 64, 511, 512, 513, 1023, 1024, 1025, 1537, 4097, 16385) + edge_lengths()
WIDE = (63, 64, 65, 257)
TRANSMATS = {"sym": SYM, "ref": REF}


def _halves(T, D, seed, gap, ld=None):
    """N(0, 1) with ``gap`` added to the first half of the rows; means [gap, 0], unit variances."""
    X = np.random.default_rng(seed).normal(size=(T, ld or D))
    X[: T // 2] += gap
    return X, np.array([[gap] * D, [0.] * D]), np.ones((2, D))


def _case(name, X, D, means, covars, transmat, startprob=HALF, n_iter=1):
    return SimpleNamespace(name=name, X=X, T=len(X), D=D, means=means, covars=covars, transmat=np.array(transmat, float),
                           startprob=np.array(startprob, float), n_iter=n_iter)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  X is what hmm_set_obs takes; D < X.shape[1] is a column prefix chosen with hmm_set_width."""
    out = []
    for T in T_GRID:
        for tag, A in TRANSMATS.items():
            X, mu, v = _halves(T, 2, [11, T], .5)
            out.append(_case("grid-%d-%s" % (T, tag), X, 2, mu, v, A))
    for T, tag in ((513, "sym"), (1025, "ref")):
        X, mu, v = _halves(T, 1, [11, T, 1], .5)
        out.append(_case("grid1-%d-%s" % (T, tag), X, 1, mu, v, TRANSMATS[tag]))
    for D in WIDE:                                          # the same total separation as .5 in two columns
        X, mu, v = _halves(700, D, [11, 700, D], .5 * np.sqrt(2. / D))
        out.append(_case("wide-%d" % D, X, D, mu, v, SYM))
    X, mu, v = _halves(1025, 2, [12, 1025], .5, ld=5)
    out.append(_case("prefix-1025", X, 2, mu, v, SYM))
    # A front that keeps a memory of row 0.  L_t[1] - L_t[0] is .25 - x for a row of two equal x: +1 at row 0, 0 at rows
    # 1 ... 5, +.7 at row 6, then -3 five times.  delta[1] - delta[0] stays at 1, inside the band of +-log 9 in which
    # (max, +) keeps it, and is 1.7 at row 6, where a back-pointer to state 1 needs more than log 9 = 2.2: the path is all
    # zeros there.  A chunk product that wrongly includes M_0 adds row 0 twice, makes it 2.7 and turns that pointer.
    for T in (512, 1025):
        X, mu, v = _halves(T, 2, [18, T], .5)
        X[0], X[1:6], X[6], X[7:12] = -.75, .25, -.45, 3.25
        out.append(_case("front-%d" % T, X, 2, mu, v, SYM))
    X, mu, v = _halves(1025, 2, [13, 1025], .5)
    out.append(_case("start10-1025", X, 2, mu, v, SYM, startprob=[1, 0]))
    out.append(_case("absorb0-1025", X, 2, mu, v, ABSORB0))
    out.append(_case("absorb1-1025", X, 2, mu, v, ABSORB1))
    out.append(_case("unreachable-1025", X, 2, mu, v, np.eye(2), startprob=[1, 0]))
    X, mu, v = _halves(1025, 2, [14, 1025], 50.)            # 50 sigma apart: exp(xi[1][0]) underflows in fp64
    out.append(_case("underflow-1025", X, 2, mu, v, SYM, n_iter=2))
    return {c.name: c for c in out}


# The unsaturated inputs: the whole T grid, the wide rows and the column prefix with the symmetric transition matrix.
# With hmm_reference.TRANSMAT (self-transition .9999) the same observations pull the posteriors to state 1 and only
# 3 % to 36 % of them stay inside [.05, .95]; those cases run as the production matrix, not as the unsaturated ones.
ESTEP_UNSATURATED = tuple(n for n in cases() if n.startswith(("grid", "wide", "prefix", "front")) and not n.endswith("-ref"))
VITERBI_CASES = tuple(n for n in cases() if n.startswith(("grid-", "absorb", "front")))


def view(case):
    """The T x D observations of a case as a contiguous copy."""
    return np.ascontiguousarray(case.X[:, :case.D])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The longdouble E-step, M-step and Viterbi of a case.  A case with n_iter = 2 is a chain: the parameters after the
    first step are rounded to fp64, which is what a device holds between iterations, and ``steps`` lists both."""
    c = cases()[name]
    X = view(c)
    mu, v, A = c.means, c.covars, c.transmat
    steps = []
    for _ in range(c.n_iter):
        L, S = emission_ld(X, mu, v)
        e = estep_ld(L, c.startprob, A)
        m = em_step_ld(X, e.gamma, e.xi, A)
        steps.append(SimpleNamespace(L=L, Sabs=S, e=e, m=m, means=mu, covars=v, transmat=A))
        mu, v, A = (np.asarray(q, dtype=np.float64) for q in (m.means, m.covars, m.transmat))
    first = steps[0]
    vit = viterbi_ld(first.L, c.startprob, c.transmat)
    return SimpleNamespace(steps=steps, L=first.L, e=steps[-1].e, m=steps[-1].m, hist=[s.e.logprob for s in steps],
                           vit=vit, u=EPS64 * max(s.e.max_alpha for s in steps))


def unsaturated_share(gamma):
    g = np.asarray(gamma[:, 0], dtype=np.float64)
    return float(np.mean((g >= .05) & (g <= .95)))


def viterbi_bound(T, vit):
    """T sequential roundings of values no larger than max |delta|."""
    return T * EPS64 * vit.max_delta


def emission_case(D):
    """One row near the first state's mean, means up to 1e3, variances from MIN_COVAR to 10: the three terms of the
    emission are near 1e9 D and cancel to about D."""
    rng = np.random.default_rng([15, D])
    means = rng.uniform(-1e3, 1e3, size=(2, D))
    covars = np.exp(rng.uniform(np.log(MIN_COVAR), np.log(10.), size=(2, D)))
    covars[:, 0] = MIN_COVAR
    means[0, 0] = 1e3
    X = means[0] + np.sqrt(covars[0]) * rng.normal(size=(1, D))
    return X, means, covars


def col_stats_case(T, D):
    return 1e6 + np.random.default_rng([16, T, D]).normal(size=(T, D))


# ---- k-means, seeding and the observation build: longdouble ----------------------------------------------------------
# The other half of a fit (k_hmm_obs, k_hmm_dist2, the Lloyd kernels, the stop rules of hicmi_hmm_kmeans and
# k_hmm_step_multi, the seeded k-means++ choice).  As above, nothing here shares code with hmm_reference.py.
def dist2_ld(X, centers):
    """d[k][t] = sum_d (X[t][d] - centers[k][d])^2 in longdouble, one row per center."""
    X = np.asarray(X).astype(LD)
    return np.stack([((X - c) ** 2).sum(axis=1) for c in np.asarray(centers).astype(LD)])


def dist_bound(D, d):
    """The derived error bound of a device distance ``d`` over D columns: a term (x - c)^2 takes at most 3 roundings, a
    lane adds ceil(D / 64) of them, the wave 6 more - (ceil(D / 64) + 9) eps64 d."""
    return (-(-D // 64) + 9) * EPS64 * d


def assign_ld(X, centers):
    """labels (ties to 0), the minimal distance and the margin |d1 - d0| of every row, and both distances (2 x T)."""
    d = dist2_ld(X, centers)
    labels = (d[1] < d[0]).astype(np.int32)
    return SimpleNamespace(labels=labels, mind=np.where(labels == 1, d[1], d[0]), margin=np.abs(d[1] - d[0]), d=d)


def label_bound(D, a):
    """Per row: what the comparison d1 < d0 of two device distances can be wrong by."""
    return dist_bound(D, a.d[0]) + dist_bound(D, a.d[1])


def cluster_means_ld(X, labels, keep):
    """(means 2 x D, scales 2 x D, counts): the longdouble mean of the rows carrying each label, ``keep[k]`` where no
    row does; scale = sum |x| / count, the magnitude the sum is formed at."""
    X = np.asarray(X).astype(LD)
    means, scale = np.array(keep).astype(LD), np.zeros((2, X.shape[1]), dtype=LD)
    counts = [int((labels == k).sum()) for k in range(2)]
    for k in range(2):
        if counts[k]:
            rows = X[labels == k]
            means[k], scale[k] = rows.sum(axis=0) / counts[k], np.abs(rows).sum(axis=0) / counts[k]
    return means, scale, counts


def lloyd_ld(X, centers, max_iter, tol):
    """Lloyd's iteration as sklearn's _kmeans_single_lloyd states it, in longdouble: labels from the centers (ties to
    0), centers from the labels (an empty cluster keeps its center); stop when no label changed ("strict"), else when
    the summed squared center shift is <= tol ("tol"), else after max_iter iterations ("max_iter"); unless the stop was
    strict, the labels returned are a last assignment from the returned centers.  ``steps`` lists, per iteration, the
    centers the assignment ran from, that assignment, the squared shift and the number of labels that changed (T in the
    first iteration)."""
    X = np.asarray(X).astype(LD)
    c = np.asarray(centers).astype(LD)
    old, steps, rule = None, [], "max_iter"
    for _ in range(int(max_iter)):
        a = assign_ld(X, c)
        new, _scale, _counts = cluster_means_ld(X, a.labels, c)
        shift = ((new - c) ** 2).sum()
        changed = len(X) if old is None else int((a.labels != old).sum())
        steps.append(SimpleNamespace(centers=c, assign=a, shift=shift, changed=changed))
        c, old = new, a.labels
        if changed == 0:
            rule = "strict"
            break
        if shift <= tol:
            rule = "tol"
            break
    final = steps[-1].assign if rule == "strict" else assign_ld(X, c)
    return SimpleNamespace(centers=c, labels=final.labels, inertia=final.mind.sum(), n_iter=len(steps), rule=rule,
                           steps=steps, final=final)


def kmeanspp_rows_ld(X, rng):
    """sklearn's greedy k-means++ for two clusters with two local trials, in longdouble, consuming ``rng`` exactly as
    scaffoldToChromosomes.kmeans_plusplus_rows does: the first row uniformly, two candidates by inverse-cdf sampling of
    the squared distances to it, the candidate with the smaller potential (the first on a tie).
    Returns rows, the two candidates, cdf_margin, gap and pot.  ``cdf_margin``: the smallest distance of a rand_vals
    entry to an entry of the cumulative sum that it could cross with a different result - all but the last one, beyond
    which the index is clamped to T - 1 anyway.  ``gap``: |pot_0 - pot_1| of the two candidates, +inf where they are the
    same row."""
    X = np.asarray(X, dtype=np.float64)
    T = len(X)
    first = int(rng.integers(T))
    closest = dist2_ld(X, X[[first]])[0]
    cum = np.cumsum(closest)
    pot = cum[-1]
    rand_vals = np.asarray(rng.uniform(size=2)).astype(LD) * pot
    cand = np.minimum(np.searchsorted(cum, rand_vals), T - 1)
    cdf_margin = min((float(np.abs(cum[:-1] - r).min()) for r in rand_vals), default=np.inf) if T > 1 else np.inf
    pots = np.minimum(closest, dist2_ld(X, X[cand])).sum(axis=1)
    gap = np.inf if cand[0] == cand[1] else float(abs(pots[0] - pots[1]))
    return SimpleNamespace(rows=[first, int(cand[int(np.argmin(pots))])], cand=[int(v) for v in cand], cdf_margin=cdf_margin,
                           gap=gap, pot=float(pot))


def seed_bound(T, D, pot):
    """What a cumulative sum or a potential formed in fp64 from device distances can be wrong by: T sequential roundings
    and the distances' own bound, at the magnitude of the potential."""
    return (T + -(-D // 64) + 9) * EPS64 * pot


def log_similarity_ld(C, order, c, p):
    """X[t][d] of hicmi_hmm_load_obs: rows order[c:], columns order[c:p].  The similarity cell is the reference's own
    fp64 expression, rounding by rounding (S2C:147-149: d = (1 - cell / numpy_row_sum) + 1, s = builtin_row_sum *
    (1 - (d - 1))), and so is the sum s + 1 that its log takes (S2C:165-183, numpy.log(matrix + 1)): those roundings are
    the definition.  The logarithm itself, log10 of that fp64 sum, is taken in longdouble; 0 where s == 0."""
    C = np.asarray(C, dtype=np.float64)
    order = np.asarray(order)
    rows, cols = order[c:], order[c:p]
    np_sum = np.add.reduce(C, axis=1)
    seq_sum = np.array([sum(r) for r in C.tolist()])
    cell = C[np.ix_(rows, cols)]
    d = (1.0 - cell / np_sum[rows, None]) + 1.0
    s = seq_sum[rows, None] * (1.0 - (d - 1.0))
    out = np.zeros(s.shape, dtype=LD)
    nz = s != 0.0
    out[nz] = np.log10((s[nz] + 1.0).astype(LD))
    return out, s


# ---- k-means in exact arithmetic ------------------------------------------------------------------------------------
def _frac_rows(A):
    return [[Fraction(v) for v in row] for row in np.asarray(A, dtype=np.float64).tolist()]


def _exact_float(q):
    f = float(q)
    assert Fraction(f) == q, "%s is not a double" % q
    return f


def lloyd_exact(X, centers, max_iter, tol):
    """lloyd_ld's statement in Python ints and fractions.Fraction: nothing is rounded.  ``centers``, ``inertia`` and
    ``shifts`` come back as doubles and the conversion is asserted to be exact, so on such data any fp64 evaluation, in
    any summation order, has to return these bits."""
    X, c = _frac_rows(X), _frac_rows(centers)
    T, tol = len(X), Fraction(tol) if np.isfinite(tol) else (Fraction(-1) if tol < 0 else None)
    old, rule, shifts, history = None, "max_iter", [], []

    def assign(c):
        d = [[sum((x - m) ** 2 for x, m in zip(row, ck)) for ck in c] for row in X]
        labels = [1 if d1 < d0 else 0 for d0, d1 in d]
        return labels, sum(dd[l] for dd, l in zip(d, labels)), sum(1 for d0, d1 in d if d0 == d1)

    ties = 0
    for _ in range(int(max_iter)):
        labels, _mind, n_tie = assign(c)
        ties += n_tie
        new = []
        for k in range(2):
            rows = [row for row, l in zip(X, labels) if l == k]
            new.append([sum(col) / len(rows) for col in zip(*rows)] if rows else c[k])
        shift = sum((a - b) ** 2 for k in range(2) for a, b in zip(new[k], c[k]))
        changed = T if old is None else sum(1 for a, b in zip(labels, old) if a != b)
        shifts.append(shift)
        history.append(labels)
        c, old = new, labels
        if changed == 0:
            rule = "strict"
            break
        if tol is None or shift <= tol:
            rule = "tol"
            break
    if rule != "strict":
        labels, _mind, n_tie = assign(c)
        ties += n_tie
    inertia = assign(c)[1] if rule != "strict" else _mind
    return SimpleNamespace(centers=np.array([[_exact_float(v) for v in ck] for ck in c]),
                           labels=np.array(labels, dtype=np.int32), inertia=_exact_float(inertia), n_iter=len(shifts),
                           rule=rule, shifts=[_exact_float(s) for s in shifts], history=history, ties=ties)


# ---- the inputs of the k-means tests (test_gpu_kmeans_steps.py) ---------------------------------------------------
KM_UNIT = 27720                                            # lcm(1 ... 12): a mean of up to 12 multiples of it is an integer
KM_MAX_ITER = 60


def col_chunks(T, D):
    """hmm_col_chunks of k_hmm.hip, restated: the row chunks a column pass over T x D is planned with."""
    col_blocks = (D + 255) // 256
    return max(1, min((2048 + col_blocks - 1) // col_blocks, 1024, T))


def col_shape(T, D):
    """hmm_col_shape of hicmi_internal.h, restated: (rows per chunk, chunks that hold rows)."""
    rows_per = -(-T // col_chunks(T, D))
    return rows_per, -(-T // rows_per)


def _pad(cols, D, where):
    """``cols`` (T x len(where)) as the columns ``where`` of a T x D matrix of zeros."""
    out = np.zeros((len(cols), D))
    out[:, list(where)] = cols
    return out


def tie_case(T, D):
    """A Lloyd fixed point with rows exactly equidistant from both centers.  Eight rows at (-4, 0), eight tie rows at
    (0, +-3), T - 16 rows at (2, 0); centers (-2, 0) and (2, 0).  A tie row is at squared distance 13 from either; with
    the tie rows in cluster 0 that cluster's mean is (-32 / 16, 0) and nothing moves.  The tie rows sit at rows 0 ... 3
    (the four waves of a k_hmm_assign workgroup), 5, 10, 15 and T - 1 (the last workgroup, partly filled unless
    T % 4 == 0).  The two informative columns are 0 and D - 1, zeros between them: D = 65 puts the second in lane 0's
    second trip, D = 257 in its fifth."""
    assert T >= 21 and D >= 2
    ties = [0, 1, 2, 3, 5, 10, 15, T - 1]
    pts = np.empty((T, 2))
    rest = [t for t in range(T) if t not in ties]
    pts[ties] = [(0, 3 if i % 2 else -3) for i in range(8)]
    pts[rest[:8]] = (-4, 0)
    pts[rest[8:]] = (2, 0)
    return _pad(pts, D, (0, D - 1)), _pad(np.array([[-2., 0.], [2., 0.]]), D, (0, D - 1)), ties


def identical_case(T, D):
    """T copies of one integer row, both centers equal to it: every distance is 0 and ties."""
    row = (np.arange(D) % 7 - 3.).reshape(1, D)
    return np.repeat(row, T, axis=0), np.repeat(row, 2, axis=0)


def exact_blobs(half, D, seed):
    """2 ``half`` rows of small integers, ``half`` (a power of two) around 0 and ``half`` around 64 in every column, in
    a seeded row order: whatever two clusters Lloyd forms of whole blobs have a power-of-two count, and every
    difference, square, sum and mean is exact in fp64 in any summation order."""
    assert half & (half - 1) == 0
    rng = np.random.default_rng([32, half, D, seed])
    X = rng.integers(-8, 9, size=(2 * half, D)).astype(np.float64)
    far = rng.permutation(2 * half)[:half]
    X[far] += 64.
    return X, np.sort(far)


def exact_scaled(T, D, seed):
    """T <= 12 rows of integers in [-20, 20] times lcm(1 ... 12): every cluster mean is an integer whatever the
    counts, and every square and sum stays far below 2^53."""
    assert T <= 12
    return np.random.default_rng([33, T, D, seed]).integers(-20, 21, size=(T, D)).astype(np.float64) * KM_UNIT


# One coordinate on which Lloyd from rows 9 and 11 changes labels in each of its first five iterations, with strictly
# decreasing squared shifts, and is strict at the sixth (asserted in test_hmm_exact_cpu.py).
STOP_COLUMN = np.array([-20, -19, -18, -15, -15, -11, -6, -4, -2, 3, 4, 13], dtype=np.float64) * KM_UNIT
STOP_ROWS = (9, 11)


def stop_case():
    """12 x 5: column 1 is STOP_COLUMN, columns 0 and 2 are zeros, columns 3 and 4 further exact data.  The width-3
    view is the stop-rule sequence (one informative column, ld 5 > D 3)."""
    X = np.zeros((12, 5))
    X[:, 1] = STOP_COLUMN
    X[:, 3:] = exact_scaled(12, 2, 0)
    return X


def chunk_labels(T, D):
    """Label 0 / 1 by the parity of the row's chunk, the other label at every chunk's first and last row."""
    rows_per, _rr = col_shape(T, D)
    t = np.arange(T)
    chunk, pos = t // rows_per, t % rows_per
    edge = (pos == 0) | (pos == rows_per - 1) | (t == T - 1)
    return ((chunk % 2) ^ edge).astype(np.int32)


CHUNK_SHAPES = ((5, 3), (1025, 3), (16385, 3), (700, 4097), (1500, 255), (1500, 256), (1500, 257))


def chunk_case(T, D):
    """Integers in [-8, 8] with column 0 set to -64 (label 0) or +64 (label 1) by chunk_labels, and centers (-64, 0, ...)
    and (64, 0, ...): the other columns cancel exactly in d1 - d0, so the first assignment is chunk_labels whatever they
    hold.  Returns X (int64), the centers, the labels, and the centers after one iteration: exact integer column sums,
    rounded once by the division."""
    rng = np.random.default_rng([34, T, D])
    X = rng.integers(-8, 9, size=(T, D))
    labels = chunk_labels(T, D)
    X[:, 0] = np.where(labels == 1, 64, -64)
    centers = np.zeros((2, D))
    centers[:, 0] = (-64., 64.)
    want = np.empty((2, D))
    for k in range(2):
        n = int((labels == k).sum())
        sums = X[labels == k].sum(axis=0, dtype=np.int64)
        want[k] = [int(s) / n for s in sums] if n else centers[k]      # int / int is correctly rounded
    return X, centers, labels, want


@functools.lru_cache(maxsize=None)
def exact_inputs():
    """name -> (X, centers, max_iter, tol): the exact-arithmetic family.  Wherever tol = 0 would end a run whose first
    shift is exactly 0 after one iteration, the same data also runs with tol = -1, which leaves the strict rule to end it."""
    out = {}
    for T in (21, 22, 23, 24):
        for D in (2, 65, 257):
            X, cen, _ties = tie_case(T, D)
            for tol in (-1., 0.):
                out["tie-%dx%d-tol%g" % (T, D, tol)] = (X, cen, 300, tol)
    for T, D in ((2, 1), (6, 65), (1025, 3)):
        X, cen = identical_case(T, D)
        for tol in (-1., 0.):
            out["identical-%dx%d-tol%g" % (T, D, tol)] = (X, cen, 300, tol)
    X, _far = exact_blobs(32, 5, 0)
    out["empty-far"] = (X, np.vstack([X[0], np.full(5, 1000.1)]), 300, 0.)
    X = exact_scaled(12, 2, 1)
    out["empty-duplicate-seeds"] = (X, X[[4, 4]], 300, 0.)
    out["empty-duplicate-seeds-1"] = (X, X[[4, 4]], 1, 0.)
    X, far = exact_blobs(64, 70, 1)
    near = np.setdiff1d(np.arange(128), far)
    out["blobs-128x70"] = (X, X[[int(far[0]), int(near[0])]], 300, 0.)
    S = stop_case()[:, :3]
    out["stop"] = (S, S[list(STOP_ROWS)], 300, 0.)
    return out


@functools.lru_cache(maxsize=None)
def exact_expected(name):
    return lloyd_exact(*exact_inputs()[name])


# -- rounded data
KM_SHAPES = ((2, 1), (2, 4097), (3, 63), (5, 4097), (1023, 256), (1024, 65), (1025, 257), (5000, 64), (16385, 1), (16385, 3))


def km_overlap(T, D, ld=None):
    """Two unit Gaussians whose means are 1.5 apart (1.5 / sqrt(D) in every column), rows of the two in seeded random
    order: many rows sit near the boundary and Lloyd runs for many iterations."""
    rng = np.random.default_rng([35, T, D])
    X = rng.normal(size=(T, ld or D))
    X[rng.permutation(T)[: T // 2]] += 1.5 / np.sqrt(D)
    return X


@functools.lru_cache(maxsize=None)
def sparse_map(n=600):
    """(contacts, order): a synthetic map rounded to two decimals with its smallest 35 % of cells set to exactly zero,
    and a seeded permutation of its rows."""
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(n, seed=4, n_chrom=3)
    C = synth.sparsify(synth.dense_contacts(lay, seed=4, sinkhorn_iters=8), .35, 2)
    return C, np.random.default_rng(36).permutation(n).astype(np.int32)


def _sparse_block(c, p):
    C, order = sparse_map()
    return np.asarray(log_similarity_ld(C, order, c, p)[0], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def km_cases():
    """name -> (X as hmm_set_obs takes it, D, the two seed rows)."""
    out = {}
    for T, D in KM_SHAPES:
        out["overlap-%dx%d" % (T, D)] = (km_overlap(T, D), D)
    out["overlap-prefix-1025x2"] = (km_overlap(1025, 2, ld=5), 2)
    out["sparse-600x257"] = (_sparse_block(0, 257), 257)
    out["sparse-300x63"] = (_sparse_block(300, 363), 63)
    out["sparse-prefix-600x64"] = (out["sparse-600x257"][0], 64)
    for name, (X, D) in list(out.items()):
        T = len(X)
        rows = np.random.default_rng([37, T, D]).choice(T, size=2, replace=False)
        out[name] = SimpleNamespace(name=name, X=X, T=T, D=D, rows=[int(r) for r in rows])
    return out


def shift_bound(c, step, nxt_scale):
    """What the squared shift of an iteration can be wrong by on a device that holds fp64 centers: each center is a mean
    of at most T terms (T eps64 scale, the sequential worst case), the shift a sum of 2 D squares of differences."""
    delta = c.T * EPS64 * float(np.sqrt((nxt_scale.astype(np.float64) ** 2).sum()))
    s = float(step.shift)
    return 4 * np.sqrt(s) * delta + 4 * delta * delta + (2 * c.D + 12) * EPS64 * s


@functools.lru_cache(maxsize=None)
def km_reference(name):
    """The longdouble trajectory of a case from its seed rows with no tolerance (strict, or KM_MAX_ITER iterations), and
    from it the runs the device is put through: name -> (max_iter, tol, iterations, rule).  ``tol`` is the geometric
    mean of the first two consecutive shifts (after the first iteration where there is one) that differ by 2 x or
    more."""
    c = km_cases()[name]
    X = view(c)
    full = lloyd_ld(X, X[c.rows], KM_MAX_ITER, -1.)
    runs = {"full": (KM_MAX_ITER, -1., full.n_iter, full.rule)}
    shifts = [float(s.shift) for s in full.steps]
    pairs = [i for i in range(len(shifts) - 1) if shifts[i] >= 2 * shifts[i + 1] > 0]
    if pairs:
        i = next((i for i in pairs if i >= 1), pairs[0])
        tol = float(np.sqrt(shifts[i] * shifts[i + 1]))
        stop = next(j for j, s in enumerate(shifts) if s <= tol)
        strict_first = next((j for j, s in enumerate(full.steps) if s.changed == 0), len(shifts))
        if stop < strict_first:
            runs["tol"] = (KM_MAX_ITER, tol, stop + 1, "tol")
    if full.n_iter > 2:
        runs["max_iter"] = (2, -1., 2, "max_iter")
    return SimpleNamespace(full=full, runs=runs, shifts=shifts)


# -- seeding
SEED_GRID = tuple((seed, 0, restart) for seed in (0, 1, 2) for restart in range(10))
SEED_CASES = ("overlap-16385x3", "sparse-600x257", "overlap-2x1")


class FixedDraws:
    """Stands in for a numpy Generator where a test dictates the draws of kmeans_plusplus_rows."""

    def __init__(self, first, uniforms):
        self.first, self.uniforms = first, np.array(uniforms, dtype=np.float64)

    def integers(self, _high):
        return self.first

    def uniform(self, size):
        assert size == len(self.uniforms)
        return self.uniforms.copy()


CLAMP_SEED = 4
CLAMP_DRAWS = (1. - 2. ** -53, .5)


def clamp_case(seed=CLAMP_SEED):
    """1000 x 1: row 0 is 0, the others (1 or 16) (1 + m 2^-25) with 25-bit m, so every squared distance to row 0 is
    exact in fp64 on any device while their sums are not.  With the first draw 1 - 2^-53 the fp64 product
    rand_vals[0] = u * sum lies above the last entry of the sequential cumulative sum when numpy's pairwise sum came out
    above it by two ulps or more, which it does for this seed (asserted where the case is used): searchsorted returns T
    and only the clamp makes it a row."""
    rng = np.random.default_rng([38, seed])
    m = rng.integers(0, 1 << 25, size=1000)
    X = np.where(rng.random(1000) < .5, 1., 16.) * (1. + m * 2. ** -25)
    X[0] = 0.
    return X.reshape(-1, 1)


def clamp_overshoot(closest):
    """By how many ulps rand_vals[0] exceeds the last cumulative sum, for the fp64 distances ``closest``."""
    pot = closest.sum()
    return float((CLAMP_DRAWS[0] * pot - np.cumsum(closest)[-1]) / np.spacing(pot))


# -- observation build: (c, p) windows of sparse_map(OBS_N) - widths 1, 255, 256, 257, T = 1, c = 0 and c = n - 1
OBS_N = 300
OBS_WINDOWS = ((0, 1), (0, 255), (0, 256), (0, 257), (43, 300), (120, 121), (299, 300))


# -- the best of ten restarts (scaffoldToChromosomes.hmm_init_params): (case, seed, fit index)
INIT_CASES = (("sparse-300x63", 0, 0), ("overlap-1024x65", 0, 0))
INIT_RESTARTS, INIT_MAX_ITER, INIT_TOL = 10, 300, 1e-4      # sklearn's n_init, max_iter, tol, as the device path has them


@functools.lru_cache(maxsize=None)
def init_reference(name, seed, fit):
    """Every restart of GaussianHMM._init's k-means in longdouble - rows from kmeanspp_rows_ld with
    default_rng([seed, fit, restart]), Lloyd from them with tol = 1e-4 mean(var(X, axis=0)) - and the winner: the
    lowest inertia, the first on a tie.  ``means`` / ``scale``: the winner's centers as the mean of the labels they were
    made of, and the magnitude those sums are formed at."""
    c = km_cases()[name]
    X = view(c)
    _mean, m2 = col_stats_ld(X)
    tol = float(INIT_TOL * (m2 / c.T).mean())
    runs = []
    for restart in range(INIT_RESTARTS):
        seeds = kmeanspp_rows_ld(X, np.random.default_rng([seed, fit, restart]))
        runs.append((seeds, lloyd_ld(X, X[seeds.rows], INIT_MAX_ITER, tol)))
    inertia = [float(r.inertia) for _s, r in runs]
    winner = int(np.argmin(inertia))
    w = runs[winner][1]
    made_of = w.labels if w.rule == "strict" else w.steps[-1].assign.labels
    means, scale, _counts = cluster_means_ld(X, made_of, w.steps[-1].centers)
    return SimpleNamespace(tol=tol, runs=runs, inertia=inertia, winner=winner, means=means, scale=scale)
