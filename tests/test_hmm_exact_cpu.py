"""The exact HMM references (hmm_exact_reference.py) without a GPU: the longdouble recursions against the sum over all
2^T paths, the fp64 restatement (hmm_reference.py) against the longdouble recursions on the inputs of the device step
tests, and the conditions those device tests rely on (test_gpu_hmm_steps.py), asserted on the same arrays."""
import itertools

import mpmath
import numpy as np
import pytest

import hmm_exact_reference as ex
import hmm_reference as ref

LD = ex.LD


def _random_model(rng, zeros):
    """startprob and transmat; with ``zeros`` some entries are exactly 0 (every row keeps a nonzero entry)."""
    pi = rng.dirichlet([1, 1])
    A = rng.dirichlet([1, 1], size=2)
    if zeros:
        if rng.random() < .5:
            k = int(rng.integers(2))
            pi = np.array([1. - k, float(k)])
        for i in range(2):
            if rng.random() < .6:
                j = int(rng.integers(2))
                A[i] = (1. - j, float(j))
    return pi, A                                            # every row keeps a nonzero entry, so some path always exists


def _brute_cases():
    rng = np.random.default_rng(21)
    out = []
    for n in range(320):
        T = 1 + n % 10
        pi, A = _random_model(rng, zeros=n % 2 == 1)
        spread = (0., 5., 50., 500.)[(n // 10) % 4]
        L = -rng.uniform(0., spread, size=(T, 2)) if spread else np.zeros((T, 2))
        out.append((L, pi, A))
    return out


def test_longdouble_recursions_equal_the_sum_over_all_paths():
    """logprob, gamma, xi and the Viterbi path of the serial longdouble recursions against brute_force.  The allowance
    is derived: an alpha or a beta is the result of at most 3 T longdouble roundings at magnitudes up to
    M = max |alpha|, and a posterior is the exponential of alpha + beta - logprob."""
    n_zero = n_unique = 0
    for L, pi, A in _brute_cases():
        T = len(L)
        lp, gamma, xi, best, best_score = ex.brute_force(L, pi, A)
        e = ex.estep_ld(L, pi, A)
        n_zero += int((np.asarray(pi) == 0).any() or (A == 0).any())
        tol = 8 * T * ex.EPS_LD * max(1., e.max_alpha)
        assert abs(e.logprob - ex.to_ld(lp)) <= tol
        g = np.array([[ex.to_ld(v) for v in row] for row in gamma])
        x = np.array([[ex.to_ld(v) for v in row] for row in xi])
        assert np.all(np.abs(e.gamma - g) <= tol * np.maximum(g, ex.EPS_LD))
        assert np.all(np.abs(e.xi - x) <= (tol + T * ex.EPS_LD) * np.maximum(x, ex.EPS_LD))
        assert np.all(e.gamma[g == 0] == 0) and np.all(e.xi[x == 0] == 0)
        v = ex.viterbi_ld(L, pi, A)
        assert tuple(int(s) for s in v.states) in best
        assert abs(v.best - ex.to_ld(best_score)) <= tol
        assert abs(ex.path_score(L, pi, A, v.states) - v.best) <= tol
        margins = np.concatenate([v.margin.ravel(), [v.final_margin]])
        if margins.min() > 2 * tol:
            assert len(best) == 1
            n_unique += 1
    assert n_zero >= 100 and n_unique >= 200


def test_every_path_is_optimal_under_exact_symmetry_and_the_rule_picks_zeros():
    for T in (1, 2, 5, 10):
        L = np.repeat(-np.random.default_rng(T).uniform(0, 9, size=(T, 1)), 2, axis=1)
        _lp, _g, _xi, best, _s = ex.brute_force(L, ex.HALF, np.full((2, 2), .5))
        assert best == set(itertools.product((0, 1), repeat=T))
        v = ex.viterbi_ld(L, ex.HALF, np.full((2, 2), .5))
        assert not v.states.any() and v.final_margin == 0 and not v.margin.any()


def test_margin_of_two_impossible_alternatives():
    v = ex.viterbi_ld(np.zeros((3, 2)), [1, 0], np.eye(2))
    assert np.all(np.isinf(v.margin[:, 1])) and np.all(np.isinf(v.margin[:, 0])) and np.isinf(v.final_margin)
    assert not v.states.any() and v.delta[2, 1] == -np.inf


def test_brute_force_on_a_case_worked_by_hand():
    """T = 2, two paths of positive weight: pi = [1, 0], A = [[.25, .75], [0, 1]], L = log [[.5, 1], [.2, .4]]."""
    L = np.log(np.array([[.5, 1.], [.2, .4]]))
    lp, gamma, xi, best, _s = ex.brute_force(L, [1, 0], [[.25, .75], [0, 1]])
    w00, w01 = .5 * .25 * .2, .5 * .75 * .4
    assert float(lp) == pytest.approx(np.log(w00 + w01), rel=1e-13)
    assert float(gamma[1][1]) == pytest.approx(w01 / (w00 + w01), rel=1e-13) and gamma[0][1] == 0
    assert float(xi[0][0]) == pytest.approx(w00 / (w00 + w01), rel=1e-13) and xi[1][1] == 0
    assert best == {(0, 1)}


def test_emission_mstep_and_column_statistics_against_mpmath():
    """The remaining longdouble operations against their formulas in mpmath on one small input each."""
    rng = np.random.default_rng(22)
    X = rng.normal(size=(5, 3)) * 10
    mu, v = rng.normal(size=(2, 3)) * 100, rng.uniform(1e-3, 2, size=(2, 3))
    L, S = ex.emission_ld(X, mu, v)
    with mpmath.workdps(50):
        mp = mpmath.mpf
        for t in range(5):
            for k in range(2):
                terms = [mpmath.log(2 * mpmath.pi) + mpmath.log(mp(v[k, d])) + (mp(X[t, d]) - mp(mu[k, d])) ** 2 / mp(v[k, d])
                         for d in range(3)]
                want = -sum(terms) / 2
                assert abs(L[t, k] - ex.to_ld(want)) <= 8 * ex.EPS_LD * S[t, k]
        g = rng.dirichlet([1, 1], size=5)
        xi = rng.uniform(size=(2, 2))
        m = ex.em_step_ld(X, g, xi, [[.5, .5], [0., 1.]])
        for k in range(2):
            post = sum(mp(g[t, k]) for t in range(5))
            for d in range(3):
                mean = sum(mp(g[t, k]) * mp(X[t, d]) for t in range(5)) / post
                var = (mp("0.01") + sum(mp(g[t, k]) * (mp(X[t, d]) - mean) ** 2 for t in range(5))) / post
                assert abs(m.means[k, d] - ex.to_ld(mean)) <= 1e-17 * float(m.means_scale[k, d])
                assert abs(m.covars[k, d] - ex.to_ld(var)) <= 1e-17 * float(m.covars_scale[k, d])
        assert np.allclose(m.transmat[0].astype(float), xi[0] / xi[0].sum(), rtol=1e-15) and list(m.transmat[1]) == [0, 1]
        Xc = 1e6 + rng.normal(size=(7, 2))
        mean, m2 = ex.col_stats_ld(Xc)
        for d in range(2):
            mu_d = sum(mp(x) for x in Xc[:, d]) / 7
            assert abs(mean[d] - ex.to_ld(mu_d)) <= 1e6 * 8 * ex.EPS_LD
            assert abs(m2[d] - ex.to_ld(sum((mp(x) - mu_d) ** 2 for x in Xc[:, d]))) <= 1e-15 * float(m2[d])
    zero = ex.em_step_ld(X, np.column_stack([np.ones(5), np.zeros(5)]), np.zeros((2, 2)), np.eye(2))
    assert np.isnan(zero.means[1]).all() and np.isnan(zero.covars[1]).all() and not np.isnan(zero.means[0]).any()
    assert np.array_equal(zero.transmat, np.zeros((2, 2)))              # zero rows are left as they are


# ---- the conditions of the device step tests ------------------------------------------------------------------------
def test_chunk_edge_lengths_come_from_the_kernel_formula():
    full, one = ex.edge_lengths()
    S = ex.chunk_steps(full)
    assert S >= 2 and full % S == 0 and full // S < 511       # thread full / S owns nothing, in mid-block
    S = ex.chunk_steps(one)
    last = (one - 1) // S
    assert S >= 2 and last < 511 and one - last * S == 1      # the last active thread owns one step
    assert full in ex.T_GRID and one in ex.T_GRID
    assert [ex.chunk_steps(T) for T in (511, 512, 513, 1024, 1025)] == [1, 1, 2, 2, 3]


def test_estep_inputs_are_unsaturated():
    """At least half of the reference posteriors of every E-step input lie in [.05, .95], and D is 1 or 2 on the T grid:
    an error at a chunk boundary then moves the posteriors, the means, the covariances and the transition matrix."""
    for name in ex.ESTEP_UNSATURATED:
        c = ex.cases()[name]
        share = ex.unsaturated_share(ex.reference(name).e.gamma)
        assert share >= .5, (name, share)
        assert c.D in (1, 2) or name.startswith("wide"), name
    assert {ex.cases()[n].T for n in ex.ESTEP_UNSATURATED} >= set(ex.T_GRID)    # every chunk shape has such an input
    for name in ex.cases():                                  # the production matrix: fewer, but never none
        if name.endswith("-ref") and ex.cases()[name].T >= 64:
            assert np.sum(np.abs(np.asarray(ex.reference(name).e.gamma[:, 0], float) - .5) <= .45) >= 20, name
    assert ex.cases()["prefix-1025"].X.shape[1] > ex.cases()["prefix-1025"].D
    for T, want in ((513, .93), (1025, .95), (4097, .90)):
        assert ex.unsaturated_share(ex.reference("grid-%d-sym" % T).e.gamma) == pytest.approx(want, abs=.01)


def test_viterbi_inputs_have_no_margin_near_the_bound():
    """Every back-pointer margin and the final-state margin of every Viterbi input exceed T eps64 max |delta|, so the
    device path must equal the reference path at every position."""
    for name in ex.VITERBI_CASES:
        c, r = ex.cases()[name], ex.reference(name)
        bound = ex.viterbi_bound(c.T, r.vit)
        m = min([float(r.vit.final_margin)] + ([float(r.vit.margin.min())] if c.T > 1 else []))
        assert m > 10 * bound, (name, m, bound)             # (the closest is 99 times the bound, at 16385 rows)


def test_zero_cases_reach_the_arithmetic_they_are_for():
    r = ex.reference("underflow-1025")
    first, second = r.steps
    assert 0 < first.m.transmat[1, 0] < LD("1e-400")             # longdouble still holds it; fp64 and its exp cannot
    assert float(np.log(first.e.xi[1, 0])) < -1000          # the device's exp(log xi) underflows whatever its rounding
    assert second.transmat[1, 0] == 0 and second.transmat[0, 1] > 0 and second.m.transmat[1, 0] == 0
    assert np.isfinite(second.e.logprob)
    r = ex.reference("unreachable-1025")
    assert r.e.gamma[:, 1].max() == 0 and np.isnan(r.m.means[1]).all() and np.isfinite(r.m.means[0]).all()
    assert np.array_equal(r.m.transmat, [[1, 0], [0, 0]])
    for name in ("absorb0-1025", "absorb1-1025", "start10-1025"):
        r = ex.reference(name)
        c = ex.cases()[name]
        assert np.isfinite(r.e.logprob) and ((c.transmat == 0).any() or (c.startprob == 0).any())
    assert np.isinf(ex.reference("start10-1025").e.alpha[0, 1])


def test_emission_inputs_cancel():
    for D in (1, 63, 64, 65, 256, 257, 4097):
        X, mu, v = ex.emission_case(D)
        L, S = ex.emission_ld(X, mu, v)
        assert v.min() == ex.MIN_COVAR and np.abs(mu).max() == 1e3
        assert float(S[0, 0] / abs(L[0, 0])) > 1e6          # state 0: terms near 1e9 cancel to about D
        assert float(abs(L[0, 0])) < 20 * D


# ---- the fp64 restatement against the longdouble recursions ------------------------------------------------------------
def _restatement_errors(name):
    c, r = ex.cases()[name], ex.reference(name)
    X = ex.view(c)
    s = r.steps[0]
    with np.errstate(all="ignore"):
        L = ref.emission(X, c.means, c.covars)
        lp, g, xi = ref.estep(L, c.startprob, c.transmat)
        mu, v, A = ref.mstep(X, g, xi, c.means, c.covars, c.transmat)
        states = ref.viterbi(X, c.means, c.covars, c.transmat, c.startprob)
    u = ex.EPS64 * s.e.max_alpha
    ok = ~np.isnan(s.m.means)
    assert np.array_equal(np.isnan(mu), ~ok) and np.array_equal(np.isnan(v), ~ok), name
    err = {"logprob": abs(lp - s.e.logprob) / u,
           "gamma": np.abs(g - s.e.gamma).max() / u,
           "xi": np.abs(xi - s.e.xi).max() / (u * max(1, c.T)),
           "means": (np.abs(mu - s.m.means)[ok] / s.m.means_scale[ok]).max() / u,
           "covars": (np.abs(v - s.m.covars)[ok] / s.m.covars_scale[ok]).max() / u,
           "transmat": np.abs(A - s.m.transmat).max() / u}
    return {k: float(e) for k, e in err.items()}, states, r.vit


# the largest error of the restatement over all cases, in units of u = eps64 max |alpha| of the case (xi: of T u), as
# measured by this test; the test allows 4 times that
RESTATEMENT_OBSERVED = {"logprob": 36.3, "gamma": .915, "xi": .276, "means": .188, "covars": .151, "transmat": .0626}


def test_restatement_is_close_to_the_longdouble_recursions():
    worst = dict.fromkeys(RESTATEMENT_OBSERVED, 0.)
    for name in ex.cases():
        err, states, vit = _restatement_errors(name)
        for k, e in err.items():
            worst[k] = max(worst[k], e)
        if name in ex.VITERBI_CASES:
            assert np.array_equal(states, vit.states), name
        print("%-18s" % name, " ".join("%s %.3g" % kv for kv in err.items()))
    print("worst", worst)
    for k, e in worst.items():
        assert e <= 4 * RESTATEMENT_OBSERVED[k], (k, e)
