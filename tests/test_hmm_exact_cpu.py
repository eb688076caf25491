"""The exact HMM references (hmm_exact_reference.py) without a GPU: the longdouble recursions against the sum over all
2^T paths, the fp64 restatement (hmm_reference.py) against the longdouble recursions on the inputs of the device step
tests, and the conditions those device tests rely on (test_gpu_hmm_steps.py), asserted on the same arrays.  Then the
same for k-means, the seeding and the observation build (test_gpu_kmeans_steps.py): the longdouble references against
exact arithmetic, the restatement against both, and the conditions on the inputs."""
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


# ---- k-means, seeding and the observation build --------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_dist2_and_lloyd_in_longdouble_equal_exact_arithmetic():
    """lloyd_ld against lloyd_exact (Python ints and Fractions) on the whole exact family, and dist2_ld against the sum
    of squares in Fractions on rounded data."""
    for name, (X, cen, max_iter, tol) in ex.exact_inputs().items():
        e, l = ex.exact_expected(name), ex.lloyd_ld(X, cen, max_iter, tol)
        assert (l.n_iter, l.rule) == (e.n_iter, e.rule), name
        assert np.array_equal(l.labels, e.labels), name
        assert np.array_equal(l.centers.astype(np.float64), e.centers) and float(l.inertia) == e.inertia, name
        assert [float(s.shift) for s in l.steps] == e.shifts, name
    rng = np.random.default_rng(23)
    X, cen = rng.normal(size=(6, 5)), rng.normal(size=(2, 5))
    d = ex.dist2_ld(X, cen)
    from fractions import Fraction as F
    for k in range(2):
        for t in range(6):
            want = sum((F(float(x)) - F(float(m))) ** 2 for x, m in zip(X[t], cen[k]))
            hi = float(d[k, t])
            got = F(hi) + F(float(d[k, t] - LD(hi)))          # a longdouble as the exact sum of two doubles
            assert abs(got - want) <= 16 * F(ex.EPS_LD) * want
    a = ex.assign_ld(X, cen)
    assert np.array_equal(a.labels, d[1] < d[0]) and np.array_equal(a.margin, np.abs(d[1] - d[0]))


def test_exact_cases_are_what_they_are_for():
    # the tie rows are exactly equidistant, stay in cluster 0, and nothing moves
    for T in (21, 22, 23, 24):
        for D in (2, 65, 257):
            X, cen, ties = ex.tie_case(T, D)
            d = ex.dist2_ld(X, cen)
            assert np.all(d[0, ties] == 13) and np.all(d[1, ties] == 13)
            others = np.setdiff1d(np.arange(T), ties)
            assert np.all(d[0, others] != d[1, others])
            assert {t % 4 for t in ties} == {0, 1, 2, 3} and T - 1 in ties
            assert D == 2 or (X[:, 1:D - 1] == 0).all() and X[:, D - 1].any()
            e = ex.lloyd_exact(X, cen, 300, -1.)
            assert (e.n_iter, e.rule) == (2, "strict") and not e.labels[ties].any() and _same_bits(e.centers, cen)
            assert e.labels.sum() == T - 16 and e.shifts == [0., 0.]
            e = ex.lloyd_exact(X, cen, 300, 0.)
            assert (e.n_iter, e.rule) == (1, "tol") and not e.labels[ties].any()
    # all rows identical: labels 0, cluster 1 empty and unmoved, inertia 0, strict at the second iteration
    X, cen = ex.identical_case(1025, 3)
    e = ex.lloyd_exact(X, cen, 300, -1.)
    assert (e.n_iter, e.rule, e.inertia) == (2, "strict", 0.) and not e.labels.any() and _same_bits(e.centers, cen)
    assert e.ties == 2 * 1025
    # a cluster that starts empty: its center comes back as it went in, the shift is the other center's alone
    X, _far = ex.exact_blobs(32, 5, 0)
    cen = np.vstack([X[0], np.full(5, 1000.1)])
    e = ex.lloyd_exact(X, cen, 300, 0.)
    assert not e.labels.any() and _same_bits(e.centers[1], cen[1]) and (e.n_iter, e.rule) == (2, "strict")
    assert _same_bits(e.centers[0], X.sum(axis=0) / 64) and e.shifts[0] == float(((X.sum(axis=0) / 64 - X[0]) ** 2).sum())
    X = ex.exact_scaled(12, 2, 1)
    e = ex.lloyd_exact(X, X[[4, 4]], 1, 0.)
    assert _same_bits(e.centers[1], X[4]) and not e.history[0].count(1) and e.ties >= 12
    assert ex.lloyd_exact(X, X[[4, 4]], 300, 0.).n_iter > 2            # ... and the run goes on from there


def test_stop_sequence_is_exact_and_changes_labels_every_iteration():
    S = ex.stop_case()[:, :3]
    cen = S[list(ex.STOP_ROWS)]
    full = ex.lloyd_exact(S, cen, 300, 0.)
    assert (full.n_iter, full.rule, full.ties) == (6, "strict", 0)
    assert all(a > b for a, b in zip(full.shifts, full.shifts[1:])) and full.shifts[-1] == 0
    assert all(full.history[k] != full.history[k + 1] for k in range(4)) and full.history[4] == full.history[5]
    for k in (1, 2, 3):                                      # tol equal to a shift stops there, the next double below not
        e = ex.lloyd_exact(S, cen, 300, full.shifts[k])
        assert (e.n_iter, e.rule) == (k + 1, "tol")
        e = ex.lloyd_exact(S, cen, 300, np.nextafter(full.shifts[k], 0.))
        assert e.n_iter == k + 2 and e.rule == ("tol" if full.shifts[k + 1] > 0 else "strict")
    for m in (1, 2, 3):                                      # the labels returned are not those the centers were made of
        e = ex.lloyd_exact(S, cen, m, 0.)
        assert (e.n_iter, e.rule) == (m, "max_iter")
        assert list(e.labels) == full.history[m] and list(e.labels) != full.history[m - 1]


def test_chunk_shapes_hit_every_edge_of_the_column_pass():
    shapes = {s: (ex.col_chunks(*s),) + ex.col_shape(*s) for s in ex.CHUNK_SHAPES}
    assert shapes[(5, 3)] == (5, 1, 5)                       # T smaller than the chunk count: one row per chunk
    R, rows_per, Rr = shapes[(1025, 3)]
    assert R == 1024 and 1025 - (Rr - 1) * rows_per == 1     # the 1024 cap; a last chunk of exactly one row
    assert shapes[(16385, 3)][0] == 1024 and shapes[(16385, 3)][1] == 17
    R, rows_per, Rr = shapes[(700, 4097)]
    assert (4097 + 255) // 256 == 17 and Rr < R              # 17 column blocks; chunks that hold no rows
    assert {D for _T, D in ex.CHUNK_SHAPES} >= {255, 256, 257}
    assert all(T * D <= 3_000_000 for T, D in ex.CHUNK_SHAPES)
    for T, D in ex.CHUNK_SHAPES:
        X, cen, labels, want = ex.chunk_case(T, D)
        rows_per, Rr = ex.col_shape(T, D)
        for ch in range(Rr):                                 # the other cluster at both ends of every chunk
            t0, t1 = ch * rows_per, min(T, (ch + 1) * rows_per)
            assert labels[t0] == labels[t1 - 1] and (t1 - t0 < 3 or labels[t0] != labels[t0 + 1])
        a = ex.assign_ld(X, cen)
        assert np.array_equal(a.labels, labels) and float(a.margin.min()) >= 4 * 64 * 64
        assert np.abs(X).max() == 64 and labels.any() and not labels.all()


def test_kmeans_inputs_meet_the_conditions_of_the_device_tests():
    """On every rounded case and every iteration of its longdouble trajectory at most 1 % of the rows have a margin
    within the distance bound (none has, and by a factor of 1e3: the trajectory is the device's own); every shift is
    further from the chosen tol than its bound; the three stop rules all occur."""
    rules = set()
    for name, c in ex.km_cases().items():
        r = ex.km_reference(name)
        X = ex.view(c)
        for s in r.full.steps + [r.full.final]:
            a = s.assign if hasattr(s, "assign") else s
            assert np.all(a.margin > 1e3 * ex.label_bound(c.D, a)), name
        for run, (max_iter, tol, n_iter, rule) in r.runs.items():
            rules.add(rule)
            got = ex.lloyd_ld(X, X[c.rows], max_iter, tol)
            assert (got.n_iter, got.rule) == (n_iter, rule), (name, run)
            for i, s in enumerate(got.steps):
                _m, scale, _n = ex.cluster_means_ld(X, s.assign.labels, s.centers)
                assert abs(float(s.shift) - tol) > 1e3 * ex.shift_bound(c, s, scale), (name, run, i)
    assert rules == {"strict", "tol", "max_iter"}
    assert sum("tol" in ex.km_reference(n).runs for n in ex.km_cases()) >= 6
    c = ex.km_cases()["overlap-1024x65"]
    assert ex.km_reference(c.name).full.n_iter >= 20          # the overlapping Gaussians do take many iterations
    X = ex.km_cases()["sparse-600x257"].X
    assert np.mean(X == 0) > .2 and len(np.unique(X)) < X.size // 3      # exact zeros, many equal cells
    assert ex.km_cases()["overlap-prefix-1025x2"].X.shape[1] == 5 and ex.km_cases()["sparse-prefix-600x64"].X.shape[1] == 257


def test_seeding_inputs_have_margins():
    """For every draw of the seeding grid the distance of a rand_vals entry to the nearest cumulative sum it could cross
    and the gap between the two candidates' potentials exceed 1e3 times the bound; the restatement picks the same rows."""
    for name in ex.SEED_CASES:
        c = ex.km_cases()[name]
        X = ex.view(c)
        for g in ex.SEED_GRID:
            r = ex.kmeanspp_rows_ld(X, np.random.default_rng(list(g)))
            bound = ex.seed_bound(c.T, c.D, r.pot)
            assert r.cdf_margin > 1e3 * bound and r.gap > 1e3 * bound, (name, g)
            assert ref.kmeans_plusplus_rows(X, np.random.default_rng(list(g))) == r.rows, (name, g)
    X = ex.clamp_case()
    assert ex.clamp_overshoot(X[:, 0] ** 2) >= 2             # searchsorted does return T here
    r = ex.kmeanspp_rows_ld(X, ex.FixedDraws(0, ex.CLAMP_DRAWS))
    assert r.cand[0] == len(X) - 1 and min(r.cdf_margin, r.gap) > 1e3 * ex.seed_bound(len(X), 1, r.pot)
    assert ref.kmeans_plusplus_rows(X, ex.FixedDraws(0, ex.CLAMP_DRAWS)) == r.rows


def test_restatement_kmeans_against_the_references():
    """hmm_reference.kmeans_lloyd bit for bit on the exact family; on rounded data its labels, iterations and stop at
    every run of the device tests, its centers to T eps64 scale, its inertia to (T + ceil(D / 64) + 9) eps64; dist2 to
    the distance bound."""
    for name, (X, cen, max_iter, tol) in ex.exact_inputs().items():
        e = ex.exact_expected(name)
        c_r, l_r, in_r, it_r = ref.kmeans_lloyd(X, cen, max_iter, tol)
        assert _same_bits(c_r, e.centers) and np.array_equal(l_r, e.labels) and it_r == e.n_iter, name
        assert _bits([in_r])[0] == _bits([e.inertia])[0], name
    for T, D in ex.CHUNK_SHAPES:
        X, cen, labels, want = ex.chunk_case(T, D)
        c_r, l_r, _in, it_r = ref.kmeans_lloyd(X.astype(np.float64), cen, 1, 0.)
        assert _same_bits(c_r, want) and np.array_equal(l_r, labels) and it_r == 1, (T, D)
    worst = 0.
    for name, c in ex.km_cases().items():
        r = ex.km_reference(name)
        X = ex.view(c)
        for run, (max_iter, tol, n_iter, rule) in r.runs.items():
            c_r, l_r, in_r, it_r = ref.kmeans_lloyd(X, X[c.rows], max_iter, tol)
            want = ex.lloyd_ld(X, X[c.rows], max_iter, tol)
            assert it_r == n_iter and np.array_equal(l_r, want.labels), (name, run)
            made_of = want.labels if rule == "strict" else want.steps[-1].assign.labels
            mean, scale, _n = ex.cluster_means_ld(X, made_of, want.steps[-1].centers)
            err = float((np.abs(c_r - mean) / (ex.EPS64 * scale)).max())
            worst = max(worst, err)
            assert err <= c.T, (name, run, err)
            at = ex.assign_ld(X, c_r)
            assert abs(in_r - at.mind.sum()) <= (c.T + -(-c.D // 64) + 9) * ex.EPS64 * float(at.mind.sum()), (name, run)
        d = ref.dist2(X, c.rows)
        want = ex.dist2_ld(X, X[c.rows])
        assert np.all(np.abs(d - want) <= (c.D + 3) * ex.EPS64 * want), name    # numpy: a pairwise sum of D terms at most
    print("restatement centers: worst error %.3g eps64 scale" % worst)


def test_log_similarity_in_longdouble():
    """log_similarity_ld against mpmath on the cells of a small window, exact zeros kept, and the fp64 restatement
    within 2 ulp of its correctly rounded values."""
    C, order = ex.sparse_map(ex.OBS_N)
    assert np.mean(C == 0) > .25 and not np.array_equal(order, np.arange(ex.OBS_N))
    A = ref.log_similarity(C, order)
    n_zero = 0
    for c, p in ex.OBS_WINDOWS:
        want, s = ex.log_similarity_ld(C, order, c, p)
        assert want.shape == (ex.OBS_N - c, p - c)
        assert np.all(want[s == 0] == 0) and np.all(want[s != 0] > 0)
        n_zero += int((s == 0).sum())
        got = A[c:, c:p]
        assert np.all(got[s == 0] == 0)
        assert np.abs(_bits(got) - _bits(want.astype(np.float64))).max() <= 2, (c, p)
    assert n_zero > 1000
    want, s = ex.log_similarity_ld(C, order, 290, 295)
    with mpmath.workdps(40):
        for i in range(10):
            for j in range(5):
                if s[i, j] != 0:
                    exact = mpmath.log10(mpmath.mpf(float(s[i, j] + 1.0)))
                    assert abs(want[i, j] - ex.to_ld(exact)) <= 4 * ex.EPS_LD * want[i, j]
    assert {p - c for c, p in ex.OBS_WINDOWS} >= {1, 255, 256, 257}
    assert {c for c, _p in ex.OBS_WINDOWS} >= {0, ex.OBS_N - 1}


def test_best_of_ten_restarts_has_one_winner():
    """The inputs of the device's initialisation test: the restarts end in different optima, the winner is not the first
    restart, its inertia is below every different one by 1e3 times what an fp64 inertia can be wrong by, every seeding
    margin and every shift's distance from tol are 1e3 bounds or more; the restatement picks the same winner."""
    for name, seed, fit in ex.INIT_CASES:
        c, r = ex.km_cases()[name], ex.init_reference(name, seed, fit)
        X = ex.view(c)
        best = r.inertia[r.winner]
        others = [v for v in r.inertia if abs(v - best) > 1e-9 * best]
        assert r.winner > 0 and len(others) >= 3, name
        assert min(others) - best > 1e3 * (c.T + -(-c.D // 64) + 9) * ex.EPS64 * best, name
        for seeds, run in r.runs:
            bound = ex.seed_bound(c.T, c.D, seeds.pot)
            assert seeds.cdf_margin > 1e3 * bound and seeds.gap > 1e3 * bound, name
            for s in run.steps:
                _m, scale, _n = ex.cluster_means_ld(X, s.assign.labels, s.centers)
                assert abs(float(s.shift) - r.tol) > 1e3 * ex.shift_bound(c, s, scale), name
                assert np.all(s.assign.margin > 1e3 * ex.label_bound(c.D, s.assign)), name
        means, _covars, _iters = ref.init_params(X, seed, fit)
        assert np.all(np.abs(means - r.means) <= c.T * ex.EPS64 * r.scale), name
