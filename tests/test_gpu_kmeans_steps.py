"""The other half of an HMM fit on the device - the observation build (k_hmm_obs), the distance pass (k_hmm_dist2), the
Lloyd iteration (k_hmm_assign, k_hmm_colsum<1> + k_hmm_combine, k_hmm_center_update, k_hmm_sum), the stop rules of
hicmi_hmm_kmeans, the seeded k-means++ choice and the lock-step kernels - against the exact references of
hmm_exact_reference.py.  Every comparison is with a reference, never with the fp64 restatement.

Exact data.  Integer-valued X on which every difference, square, sum and mean is exact in fp64 in any order: the
device has to return the bits that Python ints and Fractions give (lloyd_exact), and no tolerance appears.

Rounded data.  Each property is judged against the longdouble reference evaluated at the centers the device itself
returned.  Distances, and through them the labels, have a derived bound (dist_bound).  The two that have none:
    a center:     eps64 sum |x| / count over the rows of its cluster, per column,
    the inertia:  eps64 inertia.
ALLOW holds, per quantity, 8 times the largest error measured over all cases on an MI355X against the longdouble
reference, rounded up to a power of two (the table is in DESIGN.md section 9); no case is ever allowed more than the
sequential worst case, T roundings (the inertia: T + ceil(D / 64) + 9, its distances included).
The conditions on the inputs (margins, shifts away from tol, the seeding margins) are asserted in test_hmm_exact_cpu.py."""
import sys

import numpy as np
import pytest

import hmm_exact_reference as ex

pytestmark = pytest.mark.gpu

ALLOW = {"center": 128, "inertia": 8}                        # units above; measured 8.06 and .803


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_exact(name, got, want, labels=True):
    """(centers, labels, inertia, iterations) of the device against lloyd_exact, bit for bit."""
    cen, lab, inertia, n_iter = got
    assert n_iter == want.n_iter, (name, n_iter, want.n_iter, want.rule)
    assert np.array_equal(_bits(cen), _bits(want.centers)), (name, cen, want.centers)
    assert _bits([inertia])[0] == _bits([want.inertia])[0], (name, inertia, want.inertia)
    if labels:
        assert lab.dtype == np.int32 and np.array_equal(lab, want.labels), (name, np.flatnonzero(lab != want.labels)[:8])


# ---- exact data ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["tie", "identical", "empty", "blobs", "stop"])
def test_exact_family_bit_for_bit(family):
    """tie: rows exactly equidistant from both centers stay in cluster 0 at a fixed point, in every wave of a workgroup,
    in the last workgroup, with the deciding column in lane 0's first, second and fifth trip.  identical: every
    distance ties at 0, cluster 1 is empty and keeps its center.  empty: a cluster that is empty from the first
    assignment on (a center far outside the data; two equal seed rows) returns its center as it went in."""
    from hic_genome_assembler_amd import _lib
    names = [n for n in ex.exact_inputs() if n.startswith(family)]
    assert names
    with _lib.Context(0) as ctx:
        for name in names:
            X, cen, max_iter, tol = ex.exact_inputs()[name]
            want = ex.exact_expected(name)
            ctx.hmm_set_obs(X)
            _assert_exact(name, ctx.hmm_kmeans(cen, max_iter, tol), want)
            if family == "tie":
                ties = ex.tie_case(*X.shape)[2]
                assert want.ties >= 8 and not want.labels[ties].any()
            if name == "empty-far":
                assert np.array_equal(_bits(want.centers[1]), _bits(cen[1])) and not want.labels.any()


def test_stop_rules_on_exact_shifts():
    """The width-3 view of the 12 x 5 stop data (ld > D).  tol equal to the shift of an iteration stops there (the rule is
    <=), the next double below it does not; max_iter = 1, 2, 3 with tol = 0 stop by count, and the labels returned are
    those of the last assignment from the returned centers, which differ from the labels those centers were made of."""
    from hic_genome_assembler_amd import _lib
    S = ex.stop_case()
    V = np.ascontiguousarray(S[:, :3])
    cen = V[list(ex.STOP_ROWS)]
    shifts = ex.exact_expected("stop").shifts
    with _lib.Context(0) as ctx:
        ctx.hmm_set_obs(S)
        ctx.hmm_set_width(3)
        for k in (1, 2, 3):
            for tol in (shifts[k], float(np.nextafter(shifts[k], 0.))):
                want = ex.lloyd_exact(V, cen, 300, tol)
                assert want.n_iter == (k + 1 if tol == shifts[k] else k + 2)
                _assert_exact(("tol", k, tol), ctx.hmm_kmeans(cen, 300, tol), want)
        for max_iter in (1, 2, 3):
            want = ex.lloyd_exact(V, cen, max_iter, 0.)
            assert want.rule == "max_iter" and list(want.labels) != want.history[-1]
            _assert_exact(("max_iter", max_iter), ctx.hmm_kmeans(cen, max_iter, 0.), want)


@pytest.mark.parametrize("T,D", ex.CHUNK_SHAPES)
def test_chunk_edges_of_the_label_masked_column_pass(T, D):
    """One Lloyd iteration on integers with a row of the other cluster at every chunk's first and last row: the centers
    are the exact integer column sums, rounded once by the division.  No tolerance."""
    from hic_genome_assembler_amd import _lib
    X, cen, labels, want = ex.chunk_case(T, D)
    with _lib.Context(0) as ctx:
        ctx.hmm_set_obs(X.astype(np.float64))
        c_gpu, l_gpu, _inertia, n_iter = ctx.hmm_kmeans(cen, 1, 0.)
    bad = np.argwhere(_bits(c_gpu) != _bits(want))
    assert not len(bad), (T, D, bad[:8], c_gpu[tuple(bad[0])], want[tuple(bad[0])])
    assert n_iter == 1 and np.array_equal(l_gpu, labels)      # (the new centers still split the rows by column 0)


# ---- rounded data ----------------------------------------------------------------------------------------------------
def _load(ctx, c):
    ctx.hmm_set_obs(c.X)
    if c.D < c.X.shape[1]:
        ctx.hmm_set_width(c.D)


def _units(err, unit):
    """max err / unit; where the unit is 0 (a column of zeros) the error has to be 0 too."""
    err, unit = np.asarray(err, dtype=np.float64), np.asarray(unit, dtype=np.float64)
    assert not err[unit == 0].any()
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.


@pytest.mark.parametrize("name", list(ex.km_cases()))
def test_lloyd_on_rounded_data(name):
    from hic_genome_assembler_amd import _lib
    c, r = ex.km_cases()[name], ex.km_reference(name)
    X = ex.view(c)
    with _lib.Context(0) as ctx:
        _load(ctx, c)
        for run, (max_iter, tol, n_iter, rule) in r.runs.items():
            c_gpu, l_gpu, in_gpu, it_gpu = ctx.hmm_kmeans(X[c.rows], max_iter, tol)
            # labels: the reference's at the device's own centers, on every row whose margin exceeds the distance bound
            at = ex.assign_ld(X, c_gpu)
            safe = at.margin > ex.label_bound(c.D, at)
            assert safe.mean() >= .99, (name, run)
            assert np.array_equal(l_gpu[safe], at.labels[safe]), (name, run, np.flatnonzero(safe & (l_gpu != at.labels))[:8])
            # inertia: the sum of the minimal distances at those centers
            in_ref = at.mind.sum()
            in_err = _units(abs(in_gpu - in_ref), ex.EPS64 * in_ref)
            # iterations and the rule that stopped them (test_hmm_exact_cpu.py: no shift is near tol)
            assert it_gpu == n_iter, (name, run, it_gpu, n_iter, rule)
            # centers: the mean of the rows carrying the labels they were made of - the returned ones after a strict
            # stop, else those of the reference's last Lloyd iteration, whose later labels the device has to return
            if rule == "strict":
                made_of = l_gpu
            else:
                made_of = r.full.steps[n_iter - 1].assign.labels
                later = r.full.steps[n_iter].assign.labels if n_iter < len(r.full.steps) else r.full.final.labels
                assert np.array_equal(l_gpu, later), (name, run)
            mean, scale, counts = ex.cluster_means_ld(X, made_of, c_gpu)
            c_err = _units(np.abs(c_gpu - mean), ex.EPS64 * scale)
            print("lloyd %-22s %-8s it %2d  counts %s  center %.4g  inertia %.4g"
                  % (name, run, it_gpu, counts, c_err, in_err), file=sys.stderr)
            assert c_err <= min(ALLOW["center"], c.T), (name, run, c_err)
            assert in_err <= min(ALLOW["inertia"], c.T + -(-c.D // 64) + 9), (name, run, in_err)


@pytest.mark.parametrize("name", list(ex.km_cases()))
def test_distances_within_the_derived_bound(name):
    """hmm_dist2 to one row and to two: at most 3 roundings per term, ceil(D / 64) additions per lane, 6 for the wave."""
    from hic_genome_assembler_amd import _lib
    c = ex.km_cases()[name]
    X = ex.view(c)
    want = ex.dist2_ld(X, X[c.rows])
    with _lib.Context(0) as ctx:
        _load(ctx, c)
        for rows in (c.rows, c.rows[:1], c.rows[1:]):
            got = ctx.hmm_dist2(rows)
            w = want[[c.rows.index(r) for r in rows]]
            assert got.shape == w.shape
            assert not got[w == 0].any()                     # a row's distance to itself
            err = np.abs(got - w)
            worst = float((err[w > 0] / (ex.EPS64 * w[w > 0])).max()) if (w > 0).any() else 0.
            print("dist2 %-22s rows %d  worst %.3g eps64 dist (bound %d)" % (name, len(rows), worst, -(-c.D // 64) + 9),
                  file=sys.stderr)
            assert np.all(err <= ex.dist_bound(c.D, w)), (name, rows)


# ---- seeding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ex.SEED_CASES)
def test_seed_rows_equal_the_reference(name):
    """scaffoldToChromosomes.kmeans_plusplus_rows on the device distances, for default_rng([seed, fit, restart]) over
    3 seeds x 10 restarts, against kmeanspp_rows_ld.  No draw is excluded (test_hmm_exact_cpu.py: every margin is 1e3
    bounds or more)."""
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as p1
    c = ex.km_cases()[name]
    X = ex.view(c)
    chosen = set()
    with _lib.Context(0) as ctx:
        _load(ctx, c)
        for g in ex.SEED_GRID:
            got = p1.kmeans_plusplus_rows(c.T, ctx.hmm_dist2, np.random.default_rng(list(g)))
            want = ex.kmeanspp_rows_ld(X, np.random.default_rng(list(g)))
            assert got == want.rows, (name, g, got, want.rows)
            chosen.add(tuple(got))
    assert len(chosen) > (1 if c.T == 2 else 20)


def test_seed_candidate_beyond_the_last_cumulative_sum_is_clamped():
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as p1
    X = ex.clamp_case()
    want = ex.kmeanspp_rows_ld(X, ex.FixedDraws(0, ex.CLAMP_DRAWS))
    asked = []
    with _lib.Context(0) as ctx:
        ctx.hmm_set_obs(X)

        def dist2(rows):
            asked.append([int(r) for r in rows])
            return ctx.hmm_dist2(rows)

        assert ex.clamp_overshoot(ctx.hmm_dist2([0])[0]) >= 2    # searchsorted returns T for the first draw
        got = p1.kmeans_plusplus_rows(len(X), dist2, ex.FixedDraws(0, ex.CLAMP_DRAWS))
    assert asked == [[0], want.cand] and want.cand[0] == len(X) - 1
    assert got == want.rows


@pytest.mark.parametrize("name,seed,fit", ex.INIT_CASES)
def test_initialisation_returns_the_restart_with_the_lowest_inertia(name, seed, fit):
    """scaffoldToChromosomes.hmm_init_params: ten seeded restarts that end in different optima, of which the lowest
    inertia wins (test_hmm_exact_cpu.py: by far more than an inertia can be wrong by, and it is not the first restart).
    The means returned are the longdouble winner's."""
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as p1
    c, r = ex.km_cases()[name], ex.init_reference(name, seed, fit)
    settings = (p1.HMM_KMEANS_RESTARTS, p1.HMM_KMEANS_MAX_ITER, p1.HMM_KMEANS_TOL)
    assert settings == (ex.INIT_RESTARTS, ex.INIT_MAX_ITER, ex.INIT_TOL)
    stats = {"kmeans_iterations": 0}
    with _lib.Context(0) as ctx:
        _load(ctx, c)
        means, _covars = p1.hmm_init_params(ctx, c.T, seed, fit, stats)
    err = _units(np.abs(means - r.means), ex.EPS64 * r.scale)
    print("init %-22s winner %d of %s  center %.4g" % (name, r.winner, ["%.6g" % v for v in sorted(set(r.inertia))], err),
          file=sys.stderr)
    assert err <= min(ALLOW["center"], c.T), (name, err)
    assert stats["kmeans_iterations"] == sum(run.n_iter for _s, run in r.runs)


# ---- observation build -------------------------------------------------------------------------------------------------
def test_observations_against_the_longdouble_log_similarity():
    """hmm_load_obs on a map with exact zero cells in a permuted order: zero cells are exactly 0.0, every other cell is
    within 2 ulp of the correctly rounded log10 of the fp64 sum s + 1."""
    from hic_genome_assembler_amd import _lib
    C, order = ex.sparse_map(ex.OBS_N)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(C)
        ctx.row_sums()
        for c, p in ex.OBS_WINDOWS:
            want, s = ex.log_similarity_ld(C, order, c, p)
            assert ctx.hmm_load_obs(order, c, p) == want.shape
            X = ctx.hmm_get_obs()
            assert X.shape == want.shape
            assert not X[s == 0].any() and not np.signbit(X[s == 0]).any()
            ulps = np.abs(_bits(X) - _bits(want.astype(np.float64)))
            print("obs (%3d, %3d)  zero cells %5d  worst %d ulp" % (c, p, int((s == 0).sum()), int(ulps.max())),
                  file=sys.stderr)
            assert int(ulps.max()) <= 2, (c, p)


# ---- lock step ---------------------------------------------------------------------------------------------------------
def test_lock_step_batch_with_every_way_to_end():
    """One hmm_kmeans_multi batch whose problems end by different rules in different steps - strict at iteration 2, by
    tol at 3, by max_iter = 1, with a cluster that is empty from the start, with T = 2 - beside a problem of T > 4096,
    whose rows take the grid-stride loops of k_hmm_assign_multi / k_hmm_dist2_multi round more than once.  Every result
    equals the single call's bit for bit, and those on exact data equal lloyd_exact."""
    from hic_genome_assembler_amd import _lib
    n = 4200
    rng = np.random.default_rng(39)
    C = np.zeros((n, n))
    C[:, :8] = rng.integers(0, 50, size=(n, 8))
    C[n - 2:, n - 2:] = [[7, 3], [2, 9]]
    np.fill_diagonal(C, np.maximum(np.diag(C), 1.))
    order = np.arange(n, dtype=np.int32)
    S = ex.stop_case()
    shifts = ex.exact_expected("stop").shifts
    with _lib.Context(0) as ctx:
        ctx.set_contacts(C)
        ctx.row_sums()
        assert ctx.hmm_load_obs_slot(1, order, 0, 3) == (n, 3)
        assert ctx.hmm_load_obs_slot(2, order, n - 2, n) == (2, 2)
        ctx.hmm_set_obs(S)                                    # slot 0
        probs = [(0, 3, (0, 8), 300, 0.), (0, 3, ex.STOP_ROWS, 300, shifts[2]), (0, 3, ex.STOP_ROWS, 1, 0.),
                 (0, 5, (4, 4), 300, 0.), (0, 5, (4, 4), 1, 0.), (0, 3, ex.STOP_ROWS, 300, 0.),
                 (2, 2, (0, 1), 300, -1.), (1, 3, (17, 4100), 300, -1.), (1, 3, (17, 4100), 2, 0.)]
        got = ctx.hmm_kmeans_multi(probs)
        dist = ctx.hmm_dist2_multi([(1, 3, [4100, 17]), (2, 2, [1]), (0, 5, [4, 4])])
        ends = []
        for q, (cen, inertia, n_iter) in zip(probs, got):
            slot, width, rows, max_iter, tol = q
            ctx.hmm_use_obs(slot)
            ctx.hmm_set_width(width)
            init = np.vstack([ctx.hmm_get_obs(r, 1) for r in rows])
            c1, _lab, in1, it1 = ctx.hmm_kmeans(init, max_iter, tol)
            assert np.array_equal(_bits(cen), _bits(c1)) and _bits([inertia])[0] == _bits([in1])[0] and n_iter == it1, q
            if slot == 0:
                V = np.ascontiguousarray(S[:, :width])
                want = ex.lloyd_exact(V, V[list(rows)], max_iter, tol)
                _assert_exact(q, (cen, None, inertia, n_iter), want, labels=False)
                ends.append((want.rule, want.n_iter))
        assert ends[:3] == [("strict", 2), ("tol", 3), ("max_iter", 1)] and ends[4] == ("max_iter", 1)
        assert np.array_equal(_bits(got[4][0][1]), _bits(S[4]))              # the empty cluster's center is its seed row
        assert got[6][2] == 2 and got[7][2] >= 4 and got[8][2] == 2
        for (slot, width, rows), d in zip([(1, 3, [4100, 17]), (2, 2, [1]), (0, 5, [4, 4])], dist):
            ctx.hmm_use_obs(slot)
            ctx.hmm_set_width(width)
            assert np.array_equal(_bits(d), _bits(ctx.hmm_dist2(rows))), (slot, rows)
        want = ex.dist2_ld(S, S[[4, 4]])
        assert np.array_equal(dist[2], want.astype(np.float64))              # exact data: the distances are integers
