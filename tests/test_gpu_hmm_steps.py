"""The HMM kernels (k_hmm.hip) one step at a time against exact references (hmm_exact_reference.py): one E-step plus
M-step, the emission alone, zeros in the start probabilities and the transition matrix, Viterbi with and without ties,
and the column statistics.  Every comparison is with the longdouble reference, never with another device result.

Tolerances.  u = eps64 max |alpha_ref| of the case.  The error of logprob is absolute; that of a mean, a covariance or a
transition probability is relative to the magnitude its sums are formed at (em_step_ld's scales; a transition
probability: its value), which is the error it takes from alpha + beta through the posteriors.  ALLOW holds, per
quantity, 8 times the largest error measured over all cases on an MI355X, rounded up to a power of two, in units of u
(the table is in DESIGN.md section 9); no case is ever allowed more than T u, the worst case of T sequential roundings.
The conditions on the inputs (unsaturated posteriors, Viterbi margins) are asserted in test_hmm_exact_cpu.py."""
import math
import sys

import numpy as np
import pytest

import hmm_exact_reference as ex
import hmm_reference as ref

pytestmark = pytest.mark.gpu

ALLOW = {"logprob": 64, "means": 4, "covars": 2, "transmat": 32}      # units of u; measured 4.34, .331, .128, 2.39
ALLOW_M2 = 128                                                         # units of w (test_column_statistics); measured 13.1


def _load(ctx, c):
    ctx.hmm_set_obs(c.X)
    if c.D < c.X.shape[1]:
        ctx.hmm_set_width(c.D)


def _step_errors(c, r, got):
    """The errors of (means, covars, transmat, hist) after c.n_iter iterations, in units of u."""
    mu, v, A, hist = got
    m = r.m
    assert len(hist) == c.n_iter
    nan = np.isnan(m.means)
    assert np.array_equal(np.isnan(mu), nan) and np.array_equal(np.isnan(v), nan), c.name
    assert np.array_equal(A == 0, m.transmat.astype(np.float64) == 0), c.name
    ok = ~nan
    nz = m.transmat.astype(np.float64) != 0
    err = {"logprob": max(abs(h - w) for h, w in zip(hist, r.hist)),
           "means": (np.abs(mu - m.means)[ok] / m.means_scale[ok]).max(),
           "covars": (np.abs(v - m.covars)[ok] / m.covars_scale[ok]).max(),
           "transmat": (np.abs(A - m.transmat)[nz] / m.transmat[nz]).max() if nz.any() else 0.}
    return {k: float(e) / r.u for k, e in err.items()}


def _check_step(ctx, name):
    c, r = ex.cases()[name], ex.reference(name)
    _load(ctx, c)
    err = _step_errors(c, r, ctx.hmm_fit(c.startprob, c.means, c.covars, c.transmat, n_iter=c.n_iter, tol=-np.inf))
    print("step %-18s T %5d u %.3g  " % (name, c.T, r.u) + "  ".join("%s %.4g" % kv for kv in err.items()), file=sys.stderr)
    for k, e in err.items():
        assert e <= min(ALLOW[k], c.T), (name, k, e)


@pytest.mark.parametrize("T", ex.T_GRID)
def test_one_em_step_on_the_length_grid(T):
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        for name in ex.cases():
            if name.startswith("grid") and ex.cases()[name].T == T:
                _check_step(ctx, name)


@pytest.mark.parametrize("name", ["wide-%d" % D for D in ex.WIDE] + ["prefix-1025", "front-512", "front-1025"])
def test_one_em_step_on_wide_rows_a_column_prefix_and_a_front_that_remembers_row_0(name):
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        _check_step(ctx, name)


@pytest.mark.parametrize("name", ["start10-1025", "absorb0-1025", "absorb1-1025", "underflow-1025"])
def test_em_steps_with_zero_probabilities(name):
    """A start probability of 0, an absorbing state either way, and two iterations of which the second runs on the
    log 0 that the first one's underflow left in the transition matrix."""
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        _check_step(ctx, name)


def test_em_step_with_an_unreachable_state():
    """startprob [1, 0] and the identity: the reachable state's parameters and the logprob match the reference, the
    other state's means and covariances are NaN exactly where the restatement's are, its transition row stays zero."""
    from hic_genome_assembler_amd import _lib
    c = ex.cases()["unreachable-1025"]
    X = ex.view(c)
    with np.errstate(all="ignore"):
        _lp, g, xi = ref.estep(ref.emission(X, c.means, c.covars), c.startprob, c.transmat)
        mu_r, v_r, A_r = ref.mstep(X, g, xi, c.means, c.covars, c.transmat)
    with _lib.Context(0) as ctx:
        _load(ctx, c)
        mu, v, A, _hist = ctx.hmm_fit(c.startprob, c.means, c.covars, c.transmat, n_iter=1)
        assert np.array_equal(np.isnan(mu), np.isnan(mu_r)) and np.array_equal(np.isnan(v), np.isnan(v_r))
        assert np.isnan(mu[1]).all() and not np.isnan(mu[0]).any()
        assert np.array_equal(A, A_r) and np.array_equal(A, [[1, 0], [0, 0]])
        _check_step(ctx, c.name)


@pytest.mark.parametrize("D", [1, 63, 64, 65, 256, 257, 4097])
def test_emission_alone(D):
    """T = 1 and startprob [1, 0] (then [0, 1]): logprob is L[0][0] (then L[0][1]) itself.  Means up to 1e3, variances
    down to MIN_COVAR: terms near 1e9 D cancel.  The bound is derived: every product takes at most 3 roundings, a lane
    adds ceil(D / 64) of them, the wave 6 more, the constant and the last three operations the rest."""
    from hic_genome_assembler_amd import _lib
    X, mu, v = ex.emission_case(D)
    L, S = ex.emission_ld(X, mu, v)
    with _lib.Context(0) as ctx:
        ctx.hmm_set_obs(X)
        for k, pi in enumerate(([1, 0], [0, 1])):
            hist = ctx.hmm_fit(pi, mu, v, ex.SYM, n_iter=1)[3]
            err, bound = abs(hist[0] - L[0, k]), (math.ceil(D / 64) + 16) * ex.EPS64 * S[0, k]
            print("emission D %4d state %d  L %.17g  err %.3g  bound %.3g" % (D, k, float(L[0, k]), float(err), float(bound)),
                  file=sys.stderr)
            assert err <= bound, (D, k)


def _check_path(c, r, states):
    """The device path's score is within the bound of the optimum, and the path is the reference's."""
    bound = ex.viterbi_bound(c.T, r.vit)
    assert states.dtype == np.int32 and set(np.unique(states)) <= {0, 1}
    score = ex.path_score(r.L, c.startprob, c.transmat, states)
    assert abs(score - r.vit.best) <= bound, (c.name, float(score), float(r.vit.best))
    safe = r.vit.final_margin > bound and (c.T == 1 or r.vit.margin.min() > bound)
    assert safe, c.name                                     # (test_hmm_exact_cpu.py asserts this of the inputs)
    assert np.array_equal(states, r.vit.states), (c.name, np.flatnonzero(states != r.vit.states)[:8])
    if c.T <= 10:
        best = ex.brute_force(np.asarray(r.L, dtype=np.float64), c.startprob, c.transmat)[3]
        assert tuple(int(s) for s in states) in best


@pytest.mark.parametrize("T", ex.T_GRID)
def test_viterbi_on_the_length_grid(T):
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        for tag in ex.TRANSMATS:
            c = ex.cases()["grid-%d-%s" % (T, tag)]
            _load(ctx, c)
            _check_path(c, ex.reference(c.name), ctx.hmm_decode(c.startprob, c.means, c.covars, c.transmat))


@pytest.mark.parametrize("name", ["absorb0-1025", "absorb1-1025", "front-512", "front-1025"])
def test_viterbi_with_an_absorbing_state_and_with_a_front_that_remembers_row_0(name):
    from hic_genome_assembler_amd import _lib
    c = ex.cases()[name]
    with _lib.Context(0) as ctx:
        _load(ctx, c)
        _check_path(c, ex.reference(name), ctx.hmm_decode(c.startprob, c.means, c.covars, c.transmat))


@pytest.mark.parametrize("T", [2, 513, 1025])
def test_viterbi_exact_ties_go_to_state_zero(T):
    """Both states identical, every probability .5: every comparison in the kernel is a tie by symmetry, in the last
    state, in every back-pointer and through the suffix scan of the composed maps.  The rule gives all zeros."""
    from hic_genome_assembler_amd import _lib
    X = np.random.default_rng([17, T]).normal(size=(T, 3))
    mu, v = np.tile([.3, -.2, 1.], (2, 1)), np.tile([1., .5, 2.], (2, 1))
    with _lib.Context(0) as ctx:
        ctx.hmm_set_obs(X)
        states = ctx.hmm_decode(ex.HALF, mu, v, np.full((2, 2), .5))
    assert states.shape == (T,) and not states.any(), np.flatnonzero(states)[:8]


@pytest.mark.parametrize("T", [1, 2, 1023, 1025, 5000])
def test_column_statistics(T):
    """hmm_col_stats on columns 1e6 + N(0, 1): the mean to T eps64 1e6, the sum of squared deviations m2 to ALLOW_M2 w.
    The unit is w = eps64 m2 + T (eps64 1e6)^2: sum (x - s)^2 = m2 + T (s - mean)^2 for any shift s, and the fp64 mean the
    second pass is shifted by is no closer to the mean than one rounding at 1e6.  ALLOW_M2 is 8 times the largest error
    measured, rounded up to a power of two; no case is allowed more than (T + 2) w, its T sequential additions and the
    two roundings of a square.  A sum that is not shifted by the mean is wrong by about 1e-4 m2 here, 1e10 w."""
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        for D in (1, 255, 256, 257, 2049):
            X = ex.col_stats_case(T, D)
            mean_r, m2_r = ex.col_stats_ld(X)
            ctx.hmm_set_obs(X)
            mean, m2 = ctx.hmm_col_stats()
            assert np.abs(mean - mean_r).max() <= T * ex.EPS64 * 1e6, (T, D)
            if T == 1:
                assert not m2.any()
                continue
            w = ex.EPS64 * m2_r + T * (ex.EPS64 * 1e6) ** 2
            err = float((np.abs(m2 - m2_r) / w).max())
            print("col_stats T %4d D %4d  mean err %.3g  m2 err %.4g w" % (T, D, float(np.abs(mean - mean_r).max()), err),
                  file=sys.stderr)
            assert err <= min(ALLOW_M2, T + 2), (T, D, err)
