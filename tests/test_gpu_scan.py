"""Part 1's scan loops and the device hypergeometric test against independent references, on the GPU.

hicmi_first_pass_cuts[_multi] / hicmi_filter_cuts[_multi] (k_part1_scan.hip) and the per-scan calls hicmi_cut_scan /
hicmi_filter_scan against the oracle's pre_process_all_matrix_breakpoints / filter_noisy_breakpoints (SciPy's tail) on
planted rank matrices (tests/scan_reference.py), and the device build of hyper.h against exact integer tails on a grid
of (M, L, psig).  tests/test_scan_cpu.py shows that every case reaches its branch and that no tail the grid compares
lies within 1e-6 (relative) of psig, so everything here is compared with == and nothing is left out.

Every context first proves the planting: the device's argsort rows are the planted R.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plant(R):
    from hic_genome_assembler_amd import _lib
    ctx = _lib.Context(0)
    n = R.shape[0]
    ctx.set_contacts(sr.contacts_for_ranks(R))
    ctx.rank_matrix(np.arange(n, dtype=np.int32))           # no upgma() before it: rank_matrix sorts every row itself
    assert ctx.presort_state() == (0, 0)
    assert np.array_equal(ctx.rank_rows(), R), "the device's rank rows are not the planted ones"
    return ctx


@pytest.fixture(scope="module")
def device():
    """key -> a context that holds the planted matrix, made on first use and kept for the module."""
    made = {}

    def get(key):
        if key not in made:
            if key == "grid":
                R = sr.grid_ranks()
            elif isinstance(key, tuple):
                R = sr.mode0_ranks(key[1])
            else:
                R = sr.ranks(key)
            made[key] = _plant(R)
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


def _host_loops(monkeypatch, on):
    if on:
        monkeypatch.setenv("HICMI_HOST_SCANS", "1")
    else:
        monkeypatch.delenv("HICMI_HOST_SCANS", raising=False)


# ------------------------------------------------------------------------------------------------ loops
@pytest.mark.parametrize("case", sr.FIRST_PASS_CASES, ids=lambda c: c.name)
def test_first_pass_loop(device, monkeypatch, capsys, case):
    """Device loop, host loop and oracle: the cuts, and the (M before, M after) log against the oracle's trace."""
    from hic_genome_assembler_amd import scaffoldToChromosomes as s2c
    ref = sr.first_pass_reference(case.name)
    ctx = device(case.map)
    cuts, mlog = ctx.first_pass_cuts(case.min_size, ref.stop_ind, .05)
    assert cuts == ref.cuts, (case.name, cuts, ref.cuts)
    assert mlog == ref.mlog, (case.name, mlog, ref.mlog)
    want_lines = "\n".join(s2c.first_pass_report(ref.cuts, ref.mlog)) + "\n"
    rm = s2c.RankMatrix(ctx)
    for host in (True, False):
        _host_loops(monkeypatch, host)
        capsys.readouterr()
        got = s2c.pre_process_all_matrix_breakpoints(rm, min_size=case.min_size, min_frac=case.min_frac, psig=.05)
        assert [int(v) for v in got] == ref.cuts, (case.name, host, got)
        assert capsys.readouterr().out == want_lines, (case.name, host)


@pytest.mark.parametrize("case", sr.FILTER_CASES, ids=lambda c: c.name)
def test_filter_loop(device, monkeypatch, capsys, case):
    from hic_genome_assembler_amd import scaffoldToChromosomes as s2c
    ref = sr.filter_reference(case.name)
    ctx = device(case.map)
    kept, warned = ctx.filter_cuts(list(case.cuts), case.psig)
    assert kept == ref.kept, (case.name, kept, ref.kept)
    assert warned == ref.stats["max_rounds_exits"] == 0
    want_lines = "\n".join(s2c.filter_report(list(case.cuts), ref.kept, ref.stats["max_rounds_exits"])) + "\n"
    rm = s2c.RankMatrix(ctx)
    for host in (True, False):
        _host_loops(monkeypatch, host)
        capsys.readouterr()
        got = s2c.filter_noisy_breakpoints(rm, list(case.cuts), psig=case.psig)
        assert [int(v) for v in got] == ref.kept, (case.name, host, got)
        assert capsys.readouterr().out == want_lines, (case.name, host)


@pytest.mark.parametrize("case", sr.DUPLICATE_CASES, ids=lambda c: c.name)
def test_filter_with_duplicate_candidates_stays_on_the_host_loop(device, monkeypatch, capsys, case):
    """hicmi_filter_cuts wants ascending candidates and says so; the package keeps the per-scan loop for such a list."""
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as s2c
    ref = sr.filter_reference(case.name)
    ctx = device(case.map)
    with pytest.raises(_lib.HicmiError):
        ctx.filter_cuts(list(case.cuts), case.psig)
    _host_loops(monkeypatch, False)
    got = s2c.filter_noisy_breakpoints(s2c.RankMatrix(ctx), list(case.cuts), psig=case.psig)
    assert [int(v) for v in got] == ref.kept
    assert "WARNING" not in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ lock step
def _first_pass_sets(map_name):
    return [c for c in sr.FIRST_PASS_CASES if c.map == map_name]


def _filter_sets(map_name):
    return [c for c in sr.FILTER_CASES if c.map == map_name]


FIRST_PASS_MAPS = sorted({c.map for c in sr.FIRST_PASS_CASES})
FILTER_MAPS = sorted({c.map for c in sr.FILTER_CASES})


def _multi_first_pass(ctx, cases):
    got = ctx.first_pass_cuts_multi([(c.min_size, sr.first_pass_reference(c.name).stop_ind) for c in cases], .05)
    return [[cuts, [list(p) for p in mlog]] for cuts, mlog in got]


def _multi_filter(ctx, cases):
    got = ctx.filter_cuts_multi([list(c.cuts) for c in cases], [c.psig for c in cases])
    return [[kept, warned] for kept, warned in got]


def _want_first_pass(cases):
    return [[sr.first_pass_reference(c.name).cuts, [list(p) for p in sr.first_pass_reference(c.name).mlog]] for c in cases]


def _want_filter(cases):
    return [[sr.filter_reference(c.name).kept, 0] for c in cases]


@pytest.mark.parametrize("map_name", FIRST_PASS_MAPS)
def test_first_pass_sets_in_lock_step(device, map_name):
    """All sets of one matrix through one hicmi_first_pass_cuts_multi call, in two orders (another lead set for the
    shared counts), and each set beside itself (the same arguments: one counts for both)."""
    cases = _first_pass_sets(map_name)
    ctx = device(map_name)
    for order in (cases, cases[::-1], [cases[0]] + cases):
        assert _multi_first_pass(ctx, order) == _want_first_pass(order), (map_name, [c.name for c in order])


@pytest.mark.parametrize("map_name", FILTER_MAPS)
def test_filter_sets_in_lock_step(device, map_name):
    """The same for hicmi_filter_cuts_multi; on the 2,100-bin matrix lists below, at and above the LDS cap share a call."""
    cases = _filter_sets(map_name)
    ctx = device(map_name)
    for order in (cases, cases[::-1]):
        assert _multi_filter(ctx, order) == _want_filter(order), (map_name, [c.name for c in order])


CHILD = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_scan as t; t.child_main()"
         % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))


# a map with one set never reaches k_cut_rows_multi's sharing: the child runs those with several
SHARED_FIRST_PASS_MAPS = [m for m in FIRST_PASS_MAPS if len(_first_pass_sets(m)) > 1]
SHARED_FILTER_MAPS = [m for m in FILTER_MAPS if len(_filter_sets(m)) > 1]


def child_main():
    """The sets of every map that has several through the two lock-step calls; one JSON line per map and call."""
    for kind, maps, sets, run in (("first", SHARED_FIRST_PASS_MAPS, _first_pass_sets, _multi_first_pass),
                                  ("filter", SHARED_FILTER_MAPS, _filter_sets, _multi_filter)):
        for name in maps:
            ctx = _plant(sr.ranks(name))
            try:
                print(json.dumps({"kind": kind, "map": name, "got": run(ctx, sets(name))}))
            finally:
                ctx.close()


def test_lock_step_without_shared_counts():
    """HICMI_SCAN_SHARE=0 (every set counts its own rows) in a fresh child process: the same answers."""
    res = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ, HICMI_SCAN_SHARE="0"), capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    assert [(r["kind"], r["map"]) for r in rows] == [("first", m) for m in SHARED_FIRST_PASS_MAPS] + [("filter", m) for m in SHARED_FILTER_MAPS]
    assert len(SHARED_FIRST_PASS_MAPS) >= 3 and len(SHARED_FILTER_MAPS) == 3
    for r in rows:
        want = _want_first_pass(_first_pass_sets(r["map"])) if r["kind"] == "first" else _want_filter(_filter_sets(r["map"]))
        assert r["got"] == want, (r["kind"], r["map"])


# ------------------------------------------------------------------------------------------------ per-scan flags
def _some(entries, count=6):
    """The first and last entries and an even spread between them."""
    idx = sorted(set(np.linspace(0, len(entries) - 1, min(count, len(entries))).astype(int).tolist()))
    return [entries[i] for i in idx]


@pytest.mark.parametrize("case", sr.FIRST_PASS_CASES, ids=lambda c: c.name)
def test_first_pass_scans_one_by_one(device, case):
    """hicmi_cut_scan at the arguments of the oracle's scans: counts and flags, so a loop mismatch points at one of them."""
    ctx = device(case.map)
    for e in _some(sr.first_pass_reference(case.name).trace):
        sig, x = ctx.cut_scan(int(e["start"]), int(e["M"]), .05, want_x=True)
        assert np.array_equal(x[1:], e["x"]), (case.name, e["start"], e["M"])
        assert np.array_equal(sig, e["sig"]), (case.name, e["start"], e["M"])


@pytest.mark.parametrize("case", sr.FILTER_CASES, ids=lambda c: c.name)
def test_filter_scans_one_by_one(device, case):
    ctx = device(case.map)
    for e in _some(sr.filter_reference(case.name).trace):
        sig, x = ctx.filter_scan(int(e["start"]), int(e["c"]), len(e["x"]), int(e["M"]), case.psig, want_x=True)
        assert np.array_equal(x, e["x"]), (case.name, e["start"], e["c"])
        assert np.array_equal(sig, e["sig"]), (case.name, e["start"], e["c"])


# ------------------------------------------------------------------------------------------------ hypergeometric grid
@pytest.mark.parametrize("M", sr.GRID_M + ("extra",))
def test_device_hypergeometric_grid_filter_rule(device, M):
    """Mode 1 (flag = tail < psig, NaN -> 0): one hicmi_filter_scan(0, L, L + 1, M, psig) per grid point gives the
    device's decision for every count 0..L; all of them must equal the exact tail's.  'extra': supports that start above
    0 (2L > M) and NaN points (M < L)."""
    ctx = device("grid")
    R = sr.grid_ranks()
    points = [p for p in sr.grid_points_device() if (p in sr.GRID_EXTRA) == (M == "extra") and (M == "extra" or p[0] == M)]
    compared = 0
    for Mv, L in points:
        want_x = sr.mode1_counts(R, 0, L, L + 1)
        for psig in sr.PSIGS:
            sig, x = ctx.filter_scan(0, L, L + 1, Mv, psig, want_x=True)
            assert np.array_equal(x, want_x), (Mv, L)
            want = np.array([sr.grid_flag(int(v), Mv, L, psig, 1) for v in want_x], np.uint8)
            bad = np.flatnonzero(sig != want)
            assert bad.size == 0, (Mv, L, psig, want_x[bad][:8].tolist(), sr.grid_point(Mv, L))
            compared += len(want)
    print("M %s: %d decisions compared" % (M, compared))


@pytest.mark.parametrize("psig", sr.PSIGS)
def test_device_hypergeometric_grid_first_pass_rule(device, psig):
    """Mode 0 (flag = 0 where tail >= psig, else 1, NaN included; L = t in entry t): the matrix holds counts just below, at
    and just above the threshold of M0 in every row; hicmi_cut_scan at M0 and at two other M (one of them with NaN rows
    and supports that start above 0) against the exact tails."""
    ctx = device(("mode0", psig))
    want_x = sr.mode0_counts(sr.mode0_ranks(psig), 0)
    for Mv in sr.MODE0_M:
        sig, x = ctx.cut_scan(0, Mv, psig, want_x=True)
        assert np.array_equal(x[1:], want_x[1:]), Mv
        want = np.array([0] + [sr.grid_flag(int(want_x[t]), Mv, t, psig, 0) for t in range(1, sr.MODE0_N)], np.uint8)
        bad = np.flatnonzero(sig != want)
        assert bad.size == 0, (Mv, psig, bad[:8].tolist(), want_x[bad][:8].tolist())
