"""Exact references for the 2-state HMM kernels (k_hmm.hip) - test infrastructure only, NumPy and mpmath.

Two independent statements of the same operations, neither of which shares code with hmm_reference.py:
  * ``brute_force``: the definition itself, a sum (or a maximum) over all 2^T state paths in mpmath;
  * serial log-space forward / backward / Viterbi, the emission, one M-step and the column statistics in
    numpy.longdouble (64-bit mantissa on x86), with -inf handled explicitly.
The longdouble recursions are held to ``brute_force`` in test_hmm_exact_cpu.py; the device kernels and the fp64
restatement in hmm_reference.py are held to the longdouble recursions.

The second half of the file builds the inputs of the step tests (test_gpu_hmm_steps.py), so that the CPU suite can assert
the conditions those tests rely on (unsaturated posteriors, Viterbi margins) on exactly the same arrays.
"""
from __future__ import annotations

import functools
import itertools
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
