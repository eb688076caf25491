"""What tests/test_gpu_scan.py rests on, shown on the CPU from the references alone.

* every crafted loop case of tests/scan_reference.py reaches the branch it is named for - read off the oracle's trace;
* the exact integer tail and SciPy take the same decision at every threshold of the hypergeometric grid;
* no exact tail of the grid (nor of the first-pass threshold matrices, nor any segment test of the crafted filter
  cases) lies within 1e-6 relative of its psig: no decision the GPU test compares can hinge on rounding, so that test
  leaves nothing out.  The tail falls with x, so the two counts around each threshold bound every other count.
"""
import math
from fractions import Fraction

import numpy as np
import pytest
from scipy.stats import hypergeom

import hic_oracle as ho
import scan_reference as sr


# ------------------------------------------------------------------------------------------------ the exact tail
@pytest.mark.parametrize("M,n,N", [(10, 3, 4), (50, 20, 45), (600, 511, 511), (4096, 200, 7), (5000, 64, 3000), (65535, 1000, 1000)])
def test_exact_tail_sums_to_one_and_matches_scipy(M, n, N):
    t = sr.exact_table(M, n, N)
    assert t.S[0] == t.T == math.comb(M, N)                  # Vandermonde: the recurrence lost nothing
    assert (t.lo, t.hi) == (max(0, N - (M - n)), min(n, N))
    for x in sorted({t.lo, t.lo + 1, (t.lo + t.hi) // 2, t.hi, t.hi + 1}):
        want = float(hypergeom.sf(x - 1, M, n, N))
        got = float(sr.exact_sf(x, M, n, N))
        assert got == pytest.approx(want, rel=1e-9, abs=1e-300), (x, got, want)


def test_exact_tail_by_direct_sum():
    """Small arguments: one comb product per term."""
    for M, n, N in [(12, 5, 6), (30, 30, 7), (9, 4, 9), (21, 1, 1)]:
        for x in range(0, min(n, N) + 2):
            want = Fraction(sum(math.comb(n, k) * math.comb(M - n, N - k) for k in range(max(x, 0), min(n, N) + 1)
                                if N - k <= M - n), math.comb(M, N))
            assert sr.exact_sf(x, M, n, N) == want, (M, n, N, x)


def test_invalid_arguments_are_nan():
    for M, n, N in [(5, 6, 6), (0, 0, 0), (-3, 1, 1), (10, 11, 2), (10, 2, 11)]:
        assert sr.exact_sf(1, M, n, N) is None
        assert np.isnan(ho.hyper_geom(1, M, n, N))
    assert sr.grid_flag(3, 5, 6, .05, 0) == 1 and sr.grid_flag(3, 5, 6, .05, 1) == 0


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("M", sr.GRID_M + ("extra",))
def test_no_grid_tail_within_1e_6_of_psig_and_scipy_agrees(M):
    """The condition of the GPU grid test, with zero exclusions: at every (M, L, psig) the tails at the smallest
    significant count and the one below it - the two nearest to psig - are at least 1e-6 (relative) away from it, and
    SciPy takes the exact decisions there.  Measured on the whole grid: the closest is 7.8e-4 (M 5000, L 3000, .01)."""
    points = [p for p in sr.grid_points_cpu() if (p in sr.GRID_EXTRA) == (M == "extra") and (M == "extra" or p[0] == M)]
    assert points
    closest = 1.0
    for Mv, L in points:
        gp = sr.grid_point(Mv, L)
        if gp is None:
            assert Mv < L and np.isnan(ho.hyper_geom(1, Mv, L, L))
            continue
        for k, psig in enumerate(sr.PSIGS):
            xs = gp.x_star[k]
            assert gp.lo < xs <= gp.hi + 1
            assert gp.gap[k] >= 1e-6, (Mv, L, psig, gp.gap[k])
            closest = min(closest, gp.gap[k])
            assert float(ho.hyper_geom(xs, Mv, L, L)) < psig <= float(ho.hyper_geom(xs - 1, Mv, L, L)), (Mv, L, psig, xs)
    print("M %s: closest relative distance of a tail to its psig %.3e" % (M, closest))


def test_grid_has_supports_that_start_above_zero_and_nan_points():
    pts = sr.grid_points_device()
    assert sum(1 for M, L in pts if M < L) >= 4
    assert sum(1 for M, L in pts if L <= M < 2 * L) >= 6
    assert all(L <= sr.GRID_N // 2 for _M, L in pts)
    assert {L for _M, L in pts} >= set(sr.GRID_L_DEVICE)


def test_grid_matrix_plants_every_count():
    R = sr.grid_ranks()
    n = sr.GRID_N
    assert np.array_equal(np.sort(R[::97], axis=1), np.broadcast_to(np.arange(n), (len(R[::97]), n)))
    for L in sorted({L for _M, L in sr.grid_points_device()}):
        x = sr.mode1_counts(R, 0, L, L + 1)
        want = np.minimum(np.arange(L + 1), L)
        if L == n // 2:
            want[0] = 1                                       # n/2 ranks cannot avoid n/2 + 1 columns
        assert np.array_equal(x, want), L


@pytest.mark.parametrize("psig", sr.PSIGS)
def test_first_pass_matrix_plants_the_thresholds(psig):
    R = sr.mode0_ranks(psig)
    n, M0, k = sr.MODE0_N, sr.MODE0_M[0], sr.PSIGS.index(psig)
    assert np.array_equal(np.sort(R, axis=1), np.broadcast_to(np.arange(n), (n, n)))
    x = sr.mode0_counts(R, 0)
    aimed = np.array([sr.grid_point(M0, t).x_star[k] - 1 + (t % 3) for t in range(1, n)])
    assert np.count_nonzero(x[1:] == aimed) >= n - 1 - 4      # (a handful of rows near t = 1 and t = n - 1 are clipped)
    for off in (-1, 0, 1):                                    # below, at and above the threshold, hundreds of each
        assert np.count_nonzero(x[1:] - np.array([sr.grid_point(M0, t).x_star[k] for t in range(1, n)]) == off) > 200
    closest = 1.0
    for M in sr.MODE0_M:
        flags = [sr.grid_flag(int(x[t]), M, t, psig, 0) for t in range(1, n)]
        assert 0 < sum(flags) < n - 1
        gaps = [sr.grid_point(M, t).gap[k] for t in range(1, n) if sr.grid_point(M, t) is not None]
        closest = min(closest, min(gaps))
        if M < n - 1:
            assert all(f == 1 for f in flags[M:])             # t > M: NaN counts as significant in the first pass
    assert closest >= 1e-6, closest
    print("psig %g: closest relative distance of a threshold tail to psig %.3e" % (psig, closest))


# ------------------------------------------------------------------------------------------------ first pass
def _fp(name):
    ref = sr.first_pass_reference(name)
    return ref, sr.scans_per_start(ref.trace)


def test_first_pass_cases_cover_every_residue_of_the_segment_start():
    starts = {s % 8 for c in sr.FIRST_PASS_CASES for s, _m in _fp(c.name)[1]}
    assert starts == set(range(8))
    ends = {(e["start"] + len(e["sig"])) % 8 for c in sr.FIRST_PASS_CASES for e in _fp(c.name)[0].trace}
    assert len(ends) >= 4                                     # (n itself: the tail of the 16-byte loop)


def test_first_pass_degenerate_and_min_size_cases():
    assert _fp("n2")[0].cuts == [] and _fp("n3")[0].cuts == []
    assert _fp("n11")[0].cuts == [6]
    for name in ("n11-min-size-11", "n11-min-size-12"):       # window_size >= len: NA NA NA after one scan
        ref, scans = _fp(name)
        assert ref.cuts == [] and scans == [(0, [11])]
        assert ho.sliding_window_scores(ref.trace[0]["sig"], sr.FIRST_PASS_BY_NAME[name].min_size) is None
    ref, scans = _fp("n77-h1")
    assert len(ref.cuts) == 10 and 30 in ref.cuts and 50 in ref.cuts      # min_size 1 also cuts at the rows that break the pattern
    assert _fp("n77-h3")[0].cuts == [9, 18, 27, 36, 45, 54, 63]
    assert _fp("n131-h9")[0].cuts == [27, 44, 69, 94]         # the 9-row block 94..103 is passed over, the 10-row one too (window)


def test_first_pass_repeated_scans():
    ref, scans = _fp("n40-five-scans-same-M")
    assert scans == [(0, [40] * 5)] and ref.mlog == [(40, 40)] * 5 and ref.cuts == []
    ref, scans = _fp("n60-five-scans-nan")
    assert scans == [(0, [60]), (12, [48, 36, 24, 12, 0])]
    assert ref.mlog == [(48, 36), (36, 24), (24, 12), (12, 0), (0, -12)]
    for e in ref.trace[2:]:                                   # rows with L > M (and every row at M = 0) are NaN and count 1
        L = np.arange(1, len(e["sig"]))
        nan_rows = np.flatnonzero(L > e["M"]) if e["M"] > 0 else np.arange(len(L))
        assert len(nan_rows) >= 11
        assert np.all(np.isnan(ho.hyper_geom(e["x"][nan_rows], e["M"], L[nan_rows], L[nan_rows])))
        assert np.all(e["sig"][1:][nan_rows] == 1)
    ref, scans = _fp("n50-exactly-90%")
    assert scans == [(0, [50]), (20, [30, 10])] and ref.mlog == [(30, 10)]
    assert (int(ref.trace[1]["sig"].sum()), len(ref.trace[1]["sig"])) == (27, 30) and 27 / 30 == .9 and 27.0 / 30.0 >= .9
    ref, scans = _fp("n80-two-scans")
    assert scans == [(0, [80]), (8, [72, 64])] and ref.mlog == [(72, 64)]
    assert int(ref.trace[1]["sig"].sum()) / 72 >= .9 > int(ref.trace[2]["sig"].sum()) / 72
    assert len(_fp("n131-h4")[1][-1][1]) == 5 and _fp("n131-h4")[0].mlog[0] == (28, -75)     # M turns negative: NaN as well


def test_first_pass_last_window():
    ref, scans = _fp("n96-last-window")
    h = 6
    assert ref.cuts == [24, 48, 90] and scans[-1] == (48, [48])
    sig = ref.trace[-1]["sig"]
    scores = ho.sliding_window_scores(sig, h)
    last_full = len(sig) - 2 * h                              # the last window whose right half is complete
    assert scores[last_full] == h and list(np.flatnonzero(scores == h)) == [last_full]
    ref, scans = _fp("n96-past-last-window")
    sig = ref.trace[-1]["sig"]
    assert ref.cuts == [24, 48] and scans[-1] == (48, [48])
    assert list(sig[37:43]) == [1] * 6 and not sig[43:].any()  # the pattern is there, one position beyond the last full window
    assert ho.sliding_window_scores(sig, h)[37] == 0


def test_first_pass_loop_ends():
    ref, scans = _fp("n96-ind==stop")
    assert ref.stop_ind == 72 and ref.cuts == [24, 48, 72] and [s for s, _m in scans] == [0, 24, 48]
    ref, scans = _fp("n96-ind==stop-1")
    assert ref.stop_ind == 72 and ref.cuts == [24, 48, 71, 84] and [s for s, _m in scans] == [0, 24, 48, 71]
    ref, scans = _fp("n96-rest==min_size")
    assert ref.stop_ind == 96 and ref.cuts == [30, 60, 90] and [s for s, _m in scans] == [0, 30, 60]
    ref, scans = _fp("n96-rest==min_size+1")
    assert ref.cuts == [30, 60, 89] and scans[-1] == (89, [7])    # goes on: one more scan, of 7 rows


def test_first_pass_maps_around_the_decide_stride():
    assert _fp("n1024")[0].cuts == [300, 650] and len(_fp("n1024")[1][-1][1]) == 5
    assert _fp("n1025")[0].cuts == [301, 651]
    assert _fp("n1100")[0].cuts == [202, 547, 1030, 1075]
    assert len(_fp("n1100")[0].trace[0]["sig"]) == 1100
    ref, scans = _fp("n769-thresholds")                       # min_size 1: the first set flag followed by a clear one decides
    assert ref.cuts == [3, 144] and [s for s, _m in scans] == [0, 3, 144]


# ------------------------------------------------------------------------------------------------ filter
def _n(name):
    return sr.ranks(sr.FILTER_BY_NAME[name].map).shape[0]


@pytest.mark.parametrize("case", sr.FILTER_CASES + sr.DUPLICATE_CASES, ids=lambda c: c.name)
def test_filter_rounds_are_bounded_by_the_list(case):
    """MAX_ROUNDS (10 x the list, S2C:577) cannot be reached: a round that finds noise moves ``start`` to a candidate
    right of it (a segment's hi > lo >= start), so a pass has at most one noisy round per distinct candidate and one
    quiet round that ends it - at most len + 1 <= 10 len rounds.  The oracle's counter confirms it on every case, and
    no case for the warning exists."""
    ref = sr.filter_reference(case.name)
    assert ref.stats["max_rounds_exits"] == 0
    assert ref.stats["rounds"] <= ref.stats["passes"] * (len(set(case.cuts)) + 1)
    if _n(case.name) < 1000:                                  # (without the optional arguments: the same cuts)
        assert ref.kept == ho.filter_noisy_breakpoints(sr.ranks(case.map), list(case.cuts), psig=case.psig)


def test_filter_stats_do_not_change_the_result():
    case = sr.FILTER_BY_NAME["f120-dense"]
    assert ho.filter_noisy_breakpoints(sr.ranks(case.map), list(case.cuts), psig=case.psig) == sr.filter_reference(case.name).kept
    assert ho.filter_noisy_breakpoints(sr.ranks(case.map), [], stats={}) == []


def test_filter_branches():
    ref = sr.filter_reference("f120-one-candidate")
    assert ref.kept == [52] and len(ref.trace) == 2 and ref.stats["passes"] == 2
    # a restart lands on a candidate: the next scan has local == 0
    ref = sr.filter_reference("f120-true-cuts")
    assert sum(1 for e in ref.trace if e["start"] > 0 and e["c"] == e["start"]) >= 5
    assert all(not e["sig"].any() for e in ref.trace if e["c"] == e["start"])
    ref = sr.filter_reference("f120-zero")
    assert ref.trace[0]["start"] == 0 and ref.trace[0]["c"] == 0 and ref.kept == [0, 15, 33]
    # noise right of the scanned candidate: start jumps beyond it and the list loses more than the scanned entries
    ref = sr.filter_reference("f120-shared-later-segment")
    jumps = [(a, b) for a, b in zip(ref.trace, ref.trace[1:]) if b["start"] > a["c"] and b["start"] != a["start"]]
    assert jumps and any(len(a["altered"]) - len(b["altered"]) >= 3 for a, b in jumps)
    assert ref.kept == [20, 45, 64, 90]
    # the MD + 1 row cap, full and cut short by the end of the map
    n, MD = 120, 24
    ref = sr.filter_reference("f120-far-candidates")
    assert all(len(e["x"]) == MD + 1 and e["start"] == 0 for e in ref.trace) and ref.stats["rounds"] == 2    # no restart
    ref = sr.filter_reference("f120-dense")
    assert any(len(e["x"]) == n - e["start"] < MD + 1 for e in ref.trace)
    assert any(len(e["x"]) == MD + 1 < n - e["start"] for e in ref.trace)
    # the second pass changes the set again: a third pass (and more)
    assert ref.stats["passes"] == 4
    assert sr.filter_reference("f120-dense-.01").stats["passes"] == 5
    # psig matters
    assert sr.filter_reference("f120-noisy").kept != sr.filter_reference("f120-noisy-1e-6").kept
    for c in sr.DUPLICATE_CASES:
        assert len(set(c.cuts)) < len(c.cuts)


@pytest.mark.parametrize("count", [2047, 2048, 2049])
def test_filter_lists_around_the_lds_cap(count):
    name = "f2100-%d" % count
    ref = sr.filter_reference(name)
    assert _n(name) == 2100 and len(sr.FILTER_BY_NAME[name].cuts) == count
    lens = [len(e["altered"]) for e in ref.trace]
    assert lens[:2] == [count] * 2 and max(lens[2:]) < 2047           # two scans of the whole list (the second finds noise), then shorter ones
    assert [e["c"] for e in ref.trace[:2]] == [1, 2]
    assert not ref.trace[0]["sig"].any() and ref.trace[1]["sig"].sum() == 419
    assert len(ref.trace[1]["seg"]) == count and ref.trace[2]["start"] == 421
    assert ref.kept == [1, 421, 841, 1261, 1681, count]


def _segment_tests(name, first_round_only):
    """(x, M, local, hi - lo) of the scalar tests S2C:664-671 runs, from the trace."""
    ref = sr.filter_reference(name)
    out = []
    for e in ref.trace:
        if first_round_only and (e["start"] != 0 or e is not ref.trace[0] and e["altered"] != ref.trace[0]["altered"]):
            break
        out += [(xx, e["M"], e["c"] - e["start"], hi - lo) for lo, hi, xx in e["seg"]]
    return out


@pytest.mark.parametrize("case", sr.FILTER_CASES, ids=lambda c: c.name)
def test_no_segment_test_within_1e_6_of_psig(case):
    """The filter's scalar test hyper_geom(x, M, local, hi - lo) is the one call with n != N.  Every segment of every
    scan of the small cases (the first round of the 2,100-bin ones): the exact tail is at least 1e-6 (relative) away
    from psig, and SciPy - the oracle - decides as the exact tail does."""
    tests = sorted(set(_segment_tests(case.name, first_round_only=_n(case.name) > 1000)))
    assert tests
    assert any(local != N for _x, _M, local, N in tests) or len(case.cuts) == 1
    closest = 1.0
    for x, M, local, N in tests:
        gap = sr.exact_gap(x, M, local, N, case.psig)
        below = sr.exact_below(x, M, local, N, case.psig)
        assert gap >= sr.MARGIN, (x, M, local, N, float(gap))
        assert (float(ho.hyper_geom(x, M, local, N)) < case.psig) == below, (x, M, local, N)
        closest = min(closest, float(gap))
    print("%s: %d distinct segment tests, closest %.3e" % (case.name, len(tests), closest))
