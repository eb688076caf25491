"""Part 2's insertion phase and scan loops, step by step against the CPU oracle, on the GPU.

hicmi_p2_insert_all / _insert_all_multi / _decide_insertion / _score_insertions and hicmi_p2_scan_all / _scan_arranged
against hic_oracle.Part2Oracle (tests/insertion_reference.py drives it) on cases built to reach the data-dependent
branches of k_part2_insert.hip: the direct take, the one-bin twin rule, a short list beyond INS_MAXC with a host step
in the middle of the queue, a step whose total is 0, bit-equal candidates, more than 256 scaffolds, and arrangements
of 8191 / 8192 / 8193 bins around both LDS staging limits.  tests/test_insertion_cpu.py shows that each case reaches
its branch under the oracle alone; test_profile_counters_show_the_branch reads the library's own counters.
Arrangements and literal scores are compared with ==.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import insertion_reference as ir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_VS_LITERAL = 0.5e-9          # half of api.hip's kNearTop: what the direct take and the short-list band rest on


def _prepare(ctx, case):
    """tests/test_gpu_sweep_part2.py's _chromosome_ctx without an arrangement: every bin selected, scaffolds laid out
    over consecutive bins."""
    n = int(sum(case.lens))
    assert case.mat.shape == (n, n)
    ctx.set_contacts(case.mat)
    ctx.p2_select(np.arange(n, dtype=np.int32))
    starts = np.concatenate([[0], np.cumsum(case.lens)[:-1]]).astype(np.int32)
    ctx.p2_layout(starts, np.asarray(case.lens, np.int32))
    return ctx


@pytest.fixture(scope="module")
def device():
    """name -> a context that holds the named insertion case, made on first use and kept for the module (the 8192-bin
    matrix is uploaded once)."""
    from hic_genome_assembler_amd import _lib
    made = {}

    def get(name):
        if name not in made:
            made[name] = _prepare(_lib.Context(0), ir.ALL_CASES[name]())
        return made[name]
    yield get
    for ctx in made.values():
        ctx.close()


def _same(got, ids, rev, best, what):
    assert np.array_equal(got[0], ids) and np.array_equal(got[1], rev), (what, got[0].tolist(), got[1].tolist())
    assert got[2] == best, (what, float(got[2]).hex(), float(best).hex())


@pytest.mark.parametrize("name", sorted(ir.ALL_CASES))
def test_full_insertion(device, name):
    case, ref = ir.ALL_CASES[name](), ir.reference(name)
    _same(device(name).p2_insert_all(case.ids0, case.rev0, case.new_ids), ref.ids, ref.rev, ref.best, name)


@pytest.mark.parametrize("name", sorted(ir.ALL_CASES))
def test_every_prefix_is_a_full_insertion(device, name):
    """Each step as the final step of a shorter job: the literal pass and d.last run at every S, where the full
    insertion takes single near-top candidates directly."""
    case, ref = ir.ALL_CASES[name](), ir.reference(name)
    ctx = device(name)
    for t, s in enumerate(ref.steps):
        _same(ctx.p2_insert_all(case.ids0, case.rev0, case.new_ids[:t + 1]), s.ids, s.rev_after, s.best, (name, t))


@pytest.mark.parametrize("name", sorted(ir.ALL_CASES))
def test_one_step_decisions(device, name):
    ref = ir.reference(name)
    ctx = device(name)
    for t, s in enumerate(ref.steps):
        got = ctx.p2_decide_insertion(s.ids_before, s.rev_before, s.new_id, 0)
        want = (s.gap, s.rev, s.best) if s.decided else (-1, 0, 0.0)
        assert got == want, (name, t, got, want)


@pytest.mark.parametrize("name", ["generic", "block-diagonal-small", "isolated-1-bin"])
def test_one_step_decisions_for_a_scaffold_that_enters_flipped(device, name):
    """new_rev_now = 1: the enumeration starts with '-', so among bit-equal twins the reversed one comes first."""
    ref = ir.run_insertion(ir.ALL_CASES[name](), enter_flipped=True)
    ctx = device(name)
    for t, s in enumerate(ref.steps):
        got = ctx.p2_decide_insertion(s.ids_before, s.rev_before, s.new_id, 1)
        assert got == (s.gap, s.rev, s.best), (name, t, got)
    if name == "block-diagonal-small":
        assert all(s.rev == 1 for s in ref.steps)


@pytest.mark.parametrize("name", sorted(ir.ALL_CASES))
def test_fast_scores_against_literal_scores(device, name):
    """hicmi_p2_score_insertions (the closed form the short lists rank by) against the oracle's literal costs of the same
    step.  The direct take and the 1e-9 band are sound only while the two agree to well within the band: the bound is
    half of it, not the measured figure (about 1e-13 at these sizes; the test prints it)."""
    ref = ir.reference(name)
    ctx = device(name)
    worst = 0.0
    for t, s in enumerate(ref.steps):
        ctx.p2_set_arrangement(np.append(s.ids_before, s.new_id), np.append(s.rev_before, 0))
        total = ctx.p2_arrangement_total()
        ctx.p2_set_arrangement(s.ids_before, s.rev_before)
        fast = ctx.p2_score_insertions(s.new_id, total)
        lit = ir.by_gap_rev(s)
        ok = np.isfinite(lit)
        assert np.array_equal(np.isfinite(fast), ok), (name, t)
        if ok.any():
            worst = max(worst, float(np.max(np.abs(fast[ok] - lit[ok]) / np.abs(lit[ok]))))
    print("fast against literal, %s: largest relative difference %.3e" % (name, worst))
    assert worst < FAST_VS_LITERAL, (name, worst)


# ---------------------------------------------------------------------------------------------- lock step
# (job, case, insertions taken from it): each job runs on the context of its case, so the seven contexts are distinct
LOCK_STEP_JOBS = [("generic", "generic", 8), ("block-diagonal", "block-diagonal", 8), ("no-contacts", "no-contacts", 8),
                  ("one-step", "quantised", 1), ("two-steps", "isolated-1-bin", 2), ("three-steps", "isolated-2-bin", 3),
                  ("8192-bins", "8192-bins", 3)]


def test_lock_step_equals_single_jobs_and_the_oracle(device):
    """One hicmi_p2_insert_all_multi call: a job that never fails, one that fails at step 0 and at every later step, one
    whose totals are 0, jobs of one, two and three steps (inactive records after their last) and the 8192-bin job.  That
    one is the largest of every step, so the launches' LDS is sized by it while ``staged`` is decided per job: at steps 1
    and 2 it is beyond both staging limits, and the two- and three-step jobs run their literal pass - the final step
    always does - beside it.  Then again on the same contexts in another order: another lead, buffers reused."""
    from hic_genome_assembler_amd import _lib
    cases, refs, ctxs = {}, {}, {}
    for job, name, count in LOCK_STEP_JOBS:
        cases[job] = ir.first_steps(ir.ALL_CASES[name](), count)
        last = ir.reference(name).steps[count - 1]
        refs[job] = (last.ids, last.rev_after, last.best)
        ctxs[job] = device(name)
    assert len({id(c) for c in ctxs.values()}) == len(LOCK_STEP_JOBS)
    single = {job: ctxs[job].p2_insert_all(c.ids0, c.rev0, c.new_ids) for job, c in cases.items()}
    names = [job for job, _name, _count in LOCK_STEP_JOBS]
    for order in (names, [names[i] for i in (6, 2, 0, 5, 3, 1, 4)]):
        got = _lib.Context.p2_insert_all_multi([(ctxs[j], cases[j].ids0, cases[j].rev0, cases[j].new_ids) for j in order])
        for job, g in zip(order, got):
            _same(g, *refs[job], what=(job, order[0]))
            _same(g, *single[job], what=(job, order[0], "single"))


# ---------------------------------------------------------------------------------------------- branch reached
PROFILE_LINE = re.compile(r"insertion short lists: direct (\d+), literal with 0:(\d+) 1:(\d+) 2:(\d+) 3\+:(\d+) candidates")


def _profile_lines(device, capfd, monkeypatch, name):
    case = ir.ALL_CASES[name]()
    ctx = device(name)
    monkeypatch.setenv("HICMI_PART2_PROFILE", "1")
    capfd.readouterr()
    ctx.p2_insert_all(case.ids0, case.rev0, case.new_ids)
    err = capfd.readouterr().err
    return [tuple(int(v) for v in m.groups()) for m in PROFILE_LINE.finditer(err)]


def test_profile_counters_show_the_branch(device, capfd, monkeypatch):
    lines = _profile_lines(device, capfd, monkeypatch, "generic")
    assert len(lines) == 1 and lines[0][0] >= 1, lines                   # direct takes, one queue
    lines = _profile_lines(device, capfd, monkeypatch, "isolated-2-bin")
    assert len(lines) == 1 and lines[0][4] >= 1, lines                   # a literal list of 3 or more
    lines = _profile_lines(device, capfd, monkeypatch, "block-diagonal")
    assert len(lines) > 1, lines                                         # the queue is entered again after a host step
    lines = _profile_lines(device, capfd, monkeypatch, "block-diagonal-small")
    assert len(lines) == 1 and lines[0][4] >= 4, lines                   # lists of 5 - 8 after the twin rule; S = 8 is last


# ---------------------------------------------------------------------------------------------- process-wide switches
SWITCHES = [{"HICMI_P2_INS_MAXC": "1"}, {"HICMI_P2_INS_MAXC": "2"}, {"HICMI_P2_HOST_INSERT": "1"}, {"HICMI_P2_INSB_SPLIT": "1"}]
CHILD = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_insertion as t; t.child_main()"
         % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))


def child_main():
    """Every small case, every prefix, through hicmi_p2_insert_all; one JSON line per result."""
    from hic_genome_assembler_amd import _lib
    for name in sorted(ir.SMALL_CASES):
        case = ir.SMALL_CASES[name]()
        with _lib.Context(0) as ctx:
            _prepare(ctx, case)
            for t in range(len(case.new_ids)):
                ids, rev, best = ctx.p2_insert_all(case.ids0, case.rev0, case.new_ids[:t + 1])
                print(json.dumps({"case": name, "t": t, "ids": ids.tolist(), "rev": rev.tolist(), "best": float(best).hex()}))


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_switches_read_once_per_process(env):
    """HICMI_P2_INS_MAXC, HICMI_P2_HOST_INSERT and HICMI_P2_INSB_SPLIT are read once per process: one child each."""
    res = subprocess.run([sys.executable, "-c", CHILD], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    rows = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    want = [(name, t) for name in sorted(ir.SMALL_CASES) for t in range(len(ir.reference(name).steps))]
    assert [(r["case"], r["t"]) for r in rows] == want
    for r in rows:
        s = ir.reference(r["case"]).steps[r["t"]]
        assert r["ids"] == s.ids.tolist() and r["rev"] == s.rev_after.tolist(), (env, r["case"], r["t"])
        assert r["best"] == float(s.best).hex(), (env, r["case"], r["t"], r["best"], float(s.best).hex())


# ---------------------------------------------------------------------------------------------- scan loops
def _tables(k):
    from hic_genome_assembler_amd import orderGenome as p2
    return p2._table_arrays(k)


@pytest.mark.parametrize("name", sorted(ir.SCAN_CASES))
def test_scan_loops(name):
    from hic_genome_assembler_amd import _lib
    case, ref = ir.SCAN_CASES[name](), ir.scan_reference(name)
    orders, orients = _tables(case.k)
    with _lib.Context(0) as ctx:
        _prepare(ctx, case)
        ids, rev, best, rounds, total = ctx.p2_scan_arranged(ref.ids0, ref.rev0, case.k, orders, orients, ref.best0)
        assert total == ref.total, (name, total, ref.total)
        _same((ids, rev, best), ref.ids, ref.rev, ref.best, name)
        assert rounds == ref.rounds, (name, rounds, ref.rounds)
        # the same through hicmi_p2_scan_all, on tables and a total the caller sets up
        ctx.p2_window_tables(orders, orients)
        ctx.p2_set_arrangement(ref.ids0, ref.rev0)
        assert ctx.p2_arrangement_total() == ref.total
        ids, rev, best, _fast, rounds = ctx.p2_scan_all(ref.ids0, ref.rev0, case.k, ref.total, ref.best0, None)
        _same((ids, rev, best), ref.ids, ref.rev, ref.best, (name, "scan_all"))
        assert rounds == ref.rounds, (name, rounds, ref.rounds)


def test_scan_with_a_floor_above_every_candidate():
    from hic_genome_assembler_amd import _lib
    case, ref = ir.SCAN_CASES["probe-k3"](), ir.scan_reference("probe-k3")
    orders, orients = _tables(case.k)
    floor = 2.0 * ref.best                                               # the oracle's final best bounds every candidate it saw
    with _lib.Context(0) as ctx:
        _prepare(ctx, case)
        ctx.p2_window_tables(orders, orients)
        ids, rev, best, _fast, rounds = ctx.p2_scan_all(ref.ids0, ref.rev0, case.k, ref.total, floor, None)
        _same((ids, rev, best), ref.ids0, ref.rev0, floor, "floor")
        assert rounds == 1
