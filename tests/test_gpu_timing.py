"""The timing mode bench.py runs the library in, and the counters its roofline object is built from (run with -m gpu).

  * nn-chain counters (hicmi_nnchain_stats, the `nnchain` family's bytes) of every kernel variant against an independent
    count of SciPy's loop (tests/nnchain_count_reference.py, pinned in tests/test_timing_cpu.py);
  * results do not depend on hicmi_timing_enable: bench.py's sequence in modes 0, 1 and 2, with the pre-sort's second
    stream in use;
  * launches, bytes and milliseconds of the other families against the definitions of DESIGN.md section 4 / hicmi.h,
    stated here as formulas of n.
"""
import contextlib
import io
import os
import time

import numpy as np
import pytest

import nnchain_count_reference as ref

pytestmark = pytest.mark.gpu

SEEDS = {65: 4, 300: 5, 1025: 6, 2500: 7}            # the maps of the nn-chain parity tests (tests/test_gpu_parity.py)
NN_SWITCHES = ("HICMI_NNCHAIN_PLAIN", "HICMI_NNCHAIN_DCAP", "HICMI_NNCHAIN_NO_COMPACT", "HICMI_NNCHAIN_W1",
               "HICMI_NNCHAIN_WGS", "HICMI_NNCHAIN_GSIZE", "HICMI_NNCHAIN_W1_S", "HICMI_NNCHAIN_XCD")
FILES = ("dendrogramOrder.txt", "binGroups.txt", "assessment.txt", "chromosomeGroups.txt", "chromosomeOrders.txt",
         "plotOrder.txt")
# Timed::on() in csrc/api.hip, mode 2: the families launched a few times per map (tests/test_timing_cpu.py checks the list
# against the source and against include/hicmi.h)
FEW_LAUNCH = {"row_sums", "build_w", "nnchain", "sort_rows", "rank_invert", "presort_rows", "rank_relabel", "rank_rows_tied"}
PURE_COUNTER = "p2_window_G_flops"


@pytest.fixture(scope="module")
def hic():
    from hic_genome_assembler_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def orc():
    import hic_oracle
    return hic_oracle


_REFERENCE = {}


def _reference(orc, key, contacts):
    """(raw merges, leaves, Z of the oracle; chain steps and columns of the counting reference) - computed once per map."""
    if key not in _REFERENCE:
        dist = orc.to_distance(contacts)                         # as _upgma_both takes it: the reference walks the same chain
        zraw_r, steps, columns = ref.nn_chain_counted(dist)
        zraw_o = orc.nn_chain_raw(dist)
        assert np.array_equal(zraw_r, zraw_o)
        leaves_o, z_o = orc.average_cluster_leaves(dist)
        _REFERENCE[key] = (zraw_o, leaves_o, z_o, steps, columns)
    return _REFERENCE[key]


def _random_case(orc, n):
    c = ref.random_contacts(n, SEEDS[n])
    return c, _reference(orc, ("random", n), c)


def _set_switches(monkeypatch, env):
    for k in NN_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _run_chain(hic, contacts, calls=1):
    """timing_reset, `calls` x upgma: (leaves, Z, raw merges, nnchain_stats, timing()["nnchain"], stats after a reset)."""
    with hic.Context(0) as ctx:
        ctx.set_contacts(contacts)
        ctx.timing_reset()
        for _ in range(calls):
            leaves, z = ctx.upgma()
        zraw = ctx.raw_merges()
        st, fam = ctx.nnchain_stats(), ctx.timing()["nnchain"]
        ctx.timing_reset()
        cleared = (ctx.nnchain_stats(), ctx.timing()["nnchain"])
    return leaves, z, zraw, st, fam, cleared


def _nnchain_bytes(n, scan_columns):
    """8 B x (columns visited by the row scans + 3 x live columns per merge); merge k of n - 1 has
    n - k live columns, so the merge term is 3 * sum_{k=0}^{n-2} (n - k) = 3 (n - 1)(n + 2) / 2.  Exact in fp64 here."""
    return 8.0 * (scan_columns + 3.0 * (n - 1) * (n + 2) / 2.0)


def _check_linkage(got, expected):
    leaves, z, zraw = got
    zraw_o, leaves_o, z_o = expected
    assert np.array_equal(zraw, zraw_o) and np.array_equal(z, z_o) and np.array_equal(leaves, leaves_o)


def _counts(st):
    return (st["merges"], st["scans"], st["scan_columns"], st["cache_hits"])


# ------------------------------------------------------------------------------------------------ nn-chain counters
@pytest.mark.parametrize("no_compact", [False, True], ids=["compacting", "no-compaction"])
@pytest.mark.parametrize("dcap", [7, 64, 1024])
@pytest.mark.parametrize("n", sorted(SEEDS))
def test_plain_chain_counts_every_step_of_scipys_loop(hic, orc, monkeypatch, n, dcap, no_compact):
    """k_nn_epoch scans a row at every chain step like SciPy: its scans ARE the reference's steps and its columns the
    reference's, exactly - whatever the epoch length, and with or without compaction (the kernels count live clusters,
    total_steps + 1 - step, not the width of the matrix)."""
    env = {"HICMI_NNCHAIN_PLAIN": 1, "HICMI_NNCHAIN_DCAP": dcap}
    if no_compact:
        env["HICMI_NNCHAIN_NO_COMPACT"] = 1
    _set_switches(monkeypatch, env)
    c, (zraw_o, leaves_o, z_o, steps, columns) = _random_case(orc, n)
    leaves, z, zraw, st, fam, _cleared = _run_chain(hic, c)
    print("plain n=%d dcap=%d: %s, reference steps %d columns %d" % (n, dcap, st, steps, columns))
    _check_linkage((leaves, z, zraw), (zraw_o, leaves_o, z_o))
    assert st["scans"] == steps and st["scan_columns"] == columns
    assert st["cache_hits"] == 0
    assert st["merges"] == n - 1 and st["retries"] == 0
    assert fam["bytes"] == _nnchain_bytes(n, st["scan_columns"])
    assert fam["launches"] == -(-(n - 1) // dcap)                       # one per epoch of dcap merges


CACHED = [("default", {}),
          ("1024-lane-kernels", {"HICMI_NNCHAIN_W1": 0}),
          ("wgs1", {"HICMI_NNCHAIN_WGS": 1}), ("wgs4", {"HICMI_NNCHAIN_WGS": 4}), ("wgs8", {"HICMI_NNCHAIN_WGS": 8}),
          ("wgs16", {"HICMI_NNCHAIN_WGS": 16}), ("wgs8-gsize", {"HICMI_NNCHAIN_WGS": 8, "HICMI_NNCHAIN_GSIZE": 1}),
          ("w1-1-slice", {"HICMI_NNCHAIN_W1_S": 1}), ("w1-5-slices", {"HICMI_NNCHAIN_W1_S": 5}),
          ("w1-64-slices", {"HICMI_NNCHAIN_W1_S": 64}),
          ("spread-over-the-chip", {"HICMI_NNCHAIN_XCD": "off"}),
          # several epochs and compactions: 7 merges per epoch, 64, and 300 (what the 1024-lane kernels' own tests use)
          ("default-dcap7", {"HICMI_NNCHAIN_DCAP": 7}), ("default-dcap64", {"HICMI_NNCHAIN_DCAP": 64}),
          ("1024-lane-dcap7", {"HICMI_NNCHAIN_W1": 0, "HICMI_NNCHAIN_DCAP": 7}),
          ("wgs4-dcap7", {"HICMI_NNCHAIN_WGS": 4, "HICMI_NNCHAIN_DCAP": 7}),
          ("wgs8-gsize-dcap64", {"HICMI_NNCHAIN_WGS": 8, "HICMI_NNCHAIN_GSIZE": 1, "HICMI_NNCHAIN_DCAP": 64}),
          ("w1-5-slices-dcap64", {"HICMI_NNCHAIN_W1_S": 5, "HICMI_NNCHAIN_DCAP": 64}),
          ("w1-5-slices-dcap300-no-compaction", {"HICMI_NNCHAIN_W1_S": 5, "HICMI_NNCHAIN_DCAP": 300, "HICMI_NNCHAIN_NO_COMPACT": 1})]


def _check_cached_counts(n, st, fam, steps, columns):
    assert st["merges"] == n - 1 and st["retries"] == 0                                   # (b)
    assert st["scans"] <= steps and st["scan_columns"] <= columns                         # (c)
    assert st["cache_hits"] >= 0
    # (d) hicmi.h: cache_hits = chain steps answered by the neighbour cache instead of a scan.  The scan fused with a merge
    # is the next chain step's scan; the step that confirms a reciprocal pair is a step like any other.
    assert st["scans"] + st["cache_hits"] == steps
    assert fam["bytes"] == _nnchain_bytes(n, st["scan_columns"])


@pytest.mark.parametrize("variant", [v for _k, v in CACHED], ids=[k for k, _v in CACHED])
@pytest.mark.parametrize("n", sorted(SEEDS))
def test_cached_chain_counts_add_up_to_scipys_steps(hic, orc, monkeypatch, n, variant):
    """Every kernel with the neighbour cache - k_nn_epoch_nc, k_nn_epoch_mwc (and its GSIZE form), k_nn_epoch_w1 with 1 to 64
    replicas, on one XCD or spread out - over one or many epochs: the linkage is the oracle's (so the variant ran), and
    every chain step of SciPy's loop is counted exactly once, as a scan or as a cache hit."""
    _set_switches(monkeypatch, variant)
    c, (zraw_o, leaves_o, z_o, steps, columns) = _random_case(orc, n)
    leaves, z, zraw, st, fam, _cleared = _run_chain(hic, c)
    print("n=%d %s: %s, reference steps %d columns %d" % (n, variant, st, steps, columns))
    _check_linkage((leaves, z, zraw), (zraw_o, leaves_o, z_o))                            # (a)
    _check_cached_counts(n, st, fam, steps, columns)
    assert st["scans"] < steps                                                            # the cache answered something


def _kernel_of(switch, k, n):
    """Which kernel nn_plan (csrc/k_nnchain.hip) selects for a matrix of n columns: HICMI_NNCHAIN_WGS = k runs the
    column-sliced k_nn_epoch_mwc from 64 k columns on and the one-workgroup k_nn_epoch_nc below; HICMI_NNCHAIN_W1_S is
    always the one-wave kernel."""
    if switch == "HICMI_NNCHAIN_W1_S":
        return "k_nn_epoch_w1"
    return "k_nn_epoch_mwc" if n >= 64 * k else "k_nn_epoch_nc"


@pytest.mark.parametrize("dcap", [None, 64], ids=["planned-epochs", "dcap64"])
@pytest.mark.parametrize("switch,counts", [("HICMI_NNCHAIN_WGS", (4, 8, 16)), ("HICMI_NNCHAIN_W1_S", (1, 5, 64))],
                         ids=["column-sliced", "one-wave"])
@pytest.mark.parametrize("n", sorted(SEEDS))
def test_counts_do_not_depend_on_the_number_of_replicas(hic, orc, monkeypatch, n, switch, counts, dcap):
    """(e) The replicas of a kernel run ONE state machine: merges, scans, columns and cache hits are the same numbers for
    4, 8 and 16 workgroups of the column-sliced kernel and for 1, 5 and 64 slices of the one-wave kernel (a count added
    once per replica would scale with them).  "The same kernel": HICMI_NNCHAIN_WGS = k hands every epoch narrower than
    64 k columns to k_nn_epoch_nc, and the two kernels split the steps differently at an epoch's end (DESIGN.md section 5:
    the scan fused with an epoch's last merge is repeated by the cache rebuild, k_nn_epoch_nc has not scanned yet), so
    the widths are compared without compaction - every epoch then has the n columns of the first - and among those that
    select the same kernel; from 1,024 columns on that is all three."""
    c, _expected = _random_case(orc, n)
    seen = {}
    for k in counts:
        env = {switch: k}
        if switch == "HICMI_NNCHAIN_WGS":
            env["HICMI_NNCHAIN_NO_COMPACT"] = 1
        if dcap:
            env["HICMI_NNCHAIN_DCAP"] = dcap
        _set_switches(monkeypatch, env)
        _leaves, _z, _zraw, st, fam, _cleared = _run_chain(hic, c)
        seen.setdefault(_kernel_of(switch, k, n), {})[k] = _counts(st) + (fam["bytes"], fam["launches"])
    print("n=%d %s: %s" % (n, switch, seen))
    if n >= 1024:
        assert len(seen) == 1 and len(next(iter(seen.values()))) == 3
    for kernel, group in seen.items():
        assert len(set(group.values())) == 1, (kernel, group)


@pytest.mark.parametrize("variant", [{"HICMI_NNCHAIN_PLAIN": 1}, {}, {"HICMI_NNCHAIN_W1": 0}, {"HICMI_NNCHAIN_WGS": 8},
                                     {"HICMI_NNCHAIN_W1_S": 5, "HICMI_NNCHAIN_DCAP": 64}],
                         ids=["plain", "default", "1024-lane-kernels", "wgs8", "w1-5-slices-dcap64"])
@pytest.mark.parametrize("n", [300, 1025])
def test_counters_accumulate_between_resets_and_reset_to_zero(hic, orc, monkeypatch, n, variant):
    """Two upgma() calls between resets give exactly twice every counter of one call (the kernels' counters are zeroed per
    chain, the context's only by hicmi_timing_reset), and a reset leaves nothing behind."""
    _set_switches(monkeypatch, variant)
    c, _expected = _random_case(orc, n)
    _l, _z, zraw1, once, fam1, cleared1 = _run_chain(hic, c, calls=1)
    _l, _z, zraw2, twice, fam2, cleared2 = _run_chain(hic, c, calls=2)
    assert np.array_equal(zraw1, zraw2)
    for k in ("merges", "scans", "scan_columns", "cache_hits"):
        assert twice[k] == 2 * once[k] and once[k] == int(once[k]), k
    assert twice["retries"] == once["retries"] == 0
    assert fam2["bytes"] == 2 * fam1["bytes"] and fam2["launches"] == 2 * fam1["launches"] and fam1["launches"] >= 1
    for st, fam in (cleared1, cleared2):
        assert _counts(st) == (0, 0, 0, 0) and st["retries"] == 0
        assert fam == dict(ms=0.0, launches=0, bytes=0.0)


def _quantised(c):
    """The tie-heavy map of test_upgma_neighbour_cache_counters: one decimal, 40 % exact zeros."""
    q = np.round(c, 1)
    q[q <= np.quantile(q, 0.4)] = 0.0
    q = 0.5 * (q + q.T)
    np.fill_diagonal(q, np.maximum(np.diag(q), 1.0))
    return np.ascontiguousarray(q)


def test_counts_on_a_tie_heavy_map(hic, orc, monkeypatch):
    """Quantised sparse contacts: exact ties everywhere, so the cache must defer to a scan where SciPy's tie rule decides
    (a scan that names the previous element IS the confirming step, not one more), and a fused scan whose cache entry a
    rebuild replaces is repeated.  Every chain step is still counted once: scans + cache_hits = SciPy's steps; fewer steps
    come from the cache than on a map without ties."""
    from hic_genome_assembler_amd import synth
    _set_switches(monkeypatch, {})
    n = 1800
    lay = synth.make_layout(n, seed=5)
    q = _quantised(synth.dense_contacts(lay, seed=5, sinkhorn_iters=8))
    zraw_o, leaves_o, z_o, steps, columns = _reference(orc, ("quantised", n), q)
    leaves, z, zraw, st, fam, _cleared = _run_chain(hic, q)
    print("quantised n=%d: %s, reference steps %d columns %d" % (n, st, steps, columns))
    _check_linkage((leaves, z, zraw), (zraw_o, leaves_o, z_o))
    assert st["merges"] == n - 1 and st["retries"] == 0
    assert st["scans"] + st["cache_hits"] == steps
    assert 0 < st["scans"] and 0 <= st["cache_hits"]
    assert fam["bytes"] == _nnchain_bytes(n, st["scan_columns"])
    _set_switches(monkeypatch, {"HICMI_NNCHAIN_PLAIN": 1})
    _l, _z, zraw_p, plain, fam_p, _cleared = _run_chain(hic, q)
    assert np.array_equal(zraw_p, zraw_o)
    assert (plain["scans"], plain["scan_columns"], plain["cache_hits"]) == (steps, columns, 0)
    assert fam_p["bytes"] == _nnchain_bytes(n, columns)


# ------------------------------------------------------------------------------------------------ the benchmark's step
def _bins(lay, cls):
    return [cls(int(lay.bin_ids[k]), lay.scaffold_names[lay.scaffold_of_bin[k]], int(lay.start[k]), int(lay.stop[k]), 1.0, 0.0)
            for k in range(lay.n_bins)]


class _Job:
    """bench.py's Job.step on a small map: the resident map, Part 1 with its files written beside the device work, the
    resident Part 2 with 6 / 5 from the in-memory groups, then what the step left behind."""

    def __init__(self, hic, contacts, lay, work):
        import torch
        from hic_genome_assembler_amd.hostio import Bin
        self.lay, self.n, self.work = lay, len(contacts), str(work)
        self.ct = torch.from_numpy(np.ascontiguousarray(contacts)).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        self.bins = _bins(lay, Bin)
        self.sizes = os.path.join(self.work, "synth.sizes")
        with open(self.sizes, "w") as fh:
            fh.write("".join("%s\t%d\n" % (nm, sz) for nm, sz in zip(lay.scaffold_names, lay.scaffold_sizes_bp)))
        self.ctx = hic.Context(0)

    def f(self, k):
        return os.path.join(self.work, k)

    def step(self):
        from hic_genome_assembler_amd import orderGenome as p2, scaffoldToChromosomes as p1
        f, ctx = self.f, self.ctx
        for k in FILES:
            if os.path.exists(f(k)):
                os.remove(f(k))
        ctx.set_contacts_device(self.ct.data_ptr(), self.n, keepalive=self.ct)
        dm = p1.DeviceMatrix(ctx)
        with contextlib.redirect_stdout(io.StringIO()):
            cuts = p1.runResident(dm, list(self.bins), self.sizes, f(FILES[0]), f(FILES[1]), f(FILES[2]), f(FILES[3]), 5, 0.0,
                                  .05, overlap_files=True)
            p2.runResident(p2.GenomeMatrix(ctx), dm.kept_bins, f(FILES[3]), f(FILES[4]), f(FILES[5]), 6, 5, self.lay.resolution,
                           chromosomeList=dm.chromosome_groups, on_native_phase=dm.release_files)
            dm.finish_files()
        assert ctx.n == self.n                                       # (no empty rows: nothing was compacted away)
        zraw = ctx.raw_merges()
        with open(f(FILES[0])) as fh:
            leaves = [ln.split("\t")[0] for ln in fh.read().splitlines()]
        files = {}
        for k in FILES:
            with open(f(k), "rb") as fh:
                files[k] = fh.read()
        return dict(cuts=[int(v) for v in cuts], zraw=zraw, leaves=leaves, ranks=ctx.rank_rows(), presort=ctx.presort_state(),
                    files=files)

    def close(self):
        self.ctx.close()


def _same_step(a, b):
    assert a["cuts"] == b["cuts"]
    assert np.array_equal(a["zraw"], b["zraw"]) and a["leaves"] == b["leaves"]
    assert np.array_equal(a["ranks"], b["ranks"])
    assert a["presort"] == b["presort"]
    for k in FILES:
        assert a["files"][k] == b["files"][k], k


def _bench_sequence(hic, contacts, lay, work, mode):
    """bench.py's timed_run on one context: two steps in mode 0, timing_enable(mode), timing_reset(), two steps, timing(),
    timing_enable(False), one step.  Returns the five steps' results, the timing of the two timed steps (read twice) and
    the nn-chain counters."""
    job = _Job(hic, contacts, lay, work)
    try:
        steps = [job.step(), job.step()]
        job.ctx.timing_enable(mode)
        job.ctx.timing_reset()
        job.ctx.synchronize()
        steps += [job.step(), job.step()]
        job.ctx.synchronize()
        timing, again, stats = job.ctx.timing(), job.ctx.timing(), job.ctx.nnchain_stats()
        job.ctx.timing_enable(False)
        steps.append(job.step())
    finally:
        job.close()
    return steps, timing, again, stats


def _check_modes(runs, n, presort_expected):
    """runs: {mode: _bench_sequence(...)}, mode 0 = a context that never enabled timing."""
    first = runs[0][0][0]
    assert first["presort"][0] == presort_expected[0] and (first["presort"][1] > 0) == presort_expected[1]
    assert len(first["cuts"]) >= 3 and len(first["files"]["chromosomeOrders.txt"]) > 100
    for mode, (steps, timing, again, stats) in runs.items():
        for s in steps:
            _same_step(s, first)
        assert timing == again, "a second hicmi_timing_get added regions again"
        assert stats["merges"] == 2 * (n - 1) and stats["retries"] == 0
    names = list(runs[0][1])
    # launches and bytes are counted in every mode, and are the same numbers
    for mode in (1, 2):
        if mode not in runs:
            continue
        for k in names:
            for what in ("launches", "bytes"):
                assert runs[mode][1][k][what] == runs[0][1][k][what], (mode, k, what, runs[mode][1][k], runs[0][1][k])
        assert _counts(runs[mode][3]) == _counts(runs[0][3])
    launched = {k for k in names if runs[0][1][k]["launches"] > 0}
    print("launched:", sorted(launched))
    for mode, (_steps, timing, _again, _stats) in runs.items():
        print("mode %d ms: %s" % (mode, {k: round(v["ms"], 3) for k, v in timing.items() if v["launches"]}))
    assert {"row_sums", "build_w", "nnchain", "cut_count", "p2_select", "p2_total", "p2_window_G", "p2_window_delta"} <= launched
    assert all(v["ms"] == 0.0 for v in runs[0][1].values())
    if 1 in runs:
        for k in names:
            if k in launched and k != PURE_COUNTER:
                assert runs[1][1][k]["ms"] > 0.0, k
            else:
                assert runs[1][1][k]["ms"] == 0.0, k
    if 2 in runs:
        for k in names:
            if k in launched and k in FEW_LAUNCH:
                assert runs[2][1][k]["ms"] > 0.0, k
            else:
                assert runs[2][1][k]["ms"] == 0.0, k


def _synthetic(n, seed):
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(n, seed=seed)
    return lay, synth.dense_contacts(lay, seed=seed, sinkhorn_iters=8)


def test_results_do_not_depend_on_the_timing_mode_2100_bins(hic, tmp_path):
    """2,100 bins: above the pre-sort's default threshold of 2,048, so presort_rows and the rank_invert behind it are
    recorded on the second stream while the nn-chain runs on the first, and no multiple of 64.  The linkage, every rank row,
    the pre-sort's state, the cut indices and the bytes of the six files are the same for every step in modes 0, 1 and 2;
    launches and bytes are the same in every mode; ms is 0 in mode 0, positive for every launched family in mode 1, and in
    mode 2 positive for exactly the launched few-launch families."""
    lay, c = _synthetic(2100, 3)
    runs = {}
    for mode in (0, 1, 2):
        (tmp_path / str(mode)).mkdir()
        runs[mode] = _bench_sequence(hic, c, lay, tmp_path / str(mode), mode)
    _check_modes(runs, 2100, (1, False))
    assert runs[2][1]["presort_rows"]["launches"] == 2 and runs[2][1]["sort_rows"]["launches"] == 0


def test_results_do_not_depend_on_the_timing_mode_600_bins_presorted(hic, tmp_path, monkeypatch):
    monkeypatch.setenv("HICMI_PRESORT_FROM", "256")
    lay, c = _synthetic(600, 3)
    runs = {}
    for mode in (0, 1, 2):
        (tmp_path / str(mode)).mkdir()
        runs[mode] = _bench_sequence(hic, c, lay, tmp_path / str(mode), mode)
    _check_modes(runs, 600, (1, False))
    assert runs[1][1]["presort_rows"]["launches"] == 2


def test_results_do_not_depend_on_the_timing_mode_tied_rows(hic, tmp_path):
    """The quantised map: the pre-sort flags the rows that hold equal similarities and k_rank_rows_tied finishes them
    (its family is one of the few-launch set of mode 2, bench.py's mode)."""
    lay, c = _synthetic(2100, 3)
    q = _quantised(c)
    runs = {}
    for mode in (0, 2):
        (tmp_path / str(mode)).mkdir()
        runs[mode] = _bench_sequence(hic, q, lay, tmp_path / str(mode), mode)
    _check_modes(runs, 2100, (1, True))
    assert runs[2][1]["rank_rows_tied"]["launches"] == 2 and runs[2][1]["rank_rows_tied"]["ms"] > 0.0


# ------------------------------------------------------------------------------------------------ bytes by definition
def test_launches_and_bytes_of_a_hand_driven_sequence(hic, monkeypatch):
    """One context, one call at a time, against DESIGN.md section 4 and include/hicmi.h (e = 8 bytes, idx = 2):
        row_sums       one launch, 2 n^2 e                          = 16 n^2
        build_w        1.5 n^2 e (reads the upper triangle, writes both halves) = 12 n^2
        the row sort   n^2 (e + idx) = 10 n^2, booked to presort_rows when it ran beside the chain, else to sort_rows
        rank_invert    2 n^2 idx = 4 n^2;  rank_relabel (after a pre-sort) 2 n^2 idx = 4 n^2
        cut_count      of cut_scan(start, M): rows start + 1 .. n - 1, m = n - start - 1 of them, row start + L reads L + 1
                       uint16 entries: idx * m (m + 3) / 2; a second M on the same start re-uses the counts
        p2_select      of n2 bins: reads and writes n2^2 doubles = 16 n2^2;  p2_total: the upper triangle, 4 n2^2."""
    n = 2100
    _lay, c = _synthetic(n, 3)
    sq = float(n) * n

    def grown(ctx, before):
        now = ctx.timing()
        return now, {k: (now[k]["launches"] - before[k]["launches"], now[k]["bytes"] - before[k]["bytes"])
                     for k in now if now[k]["launches"] != before[k]["launches"] or now[k]["bytes"] != before[k]["bytes"]}

    for presort in (True, False):
        if presort:
            monkeypatch.delenv("HICMI_NO_PRESORT", raising=False)
        else:
            monkeypatch.setenv("HICMI_NO_PRESORT", "1")
        with hic.Context(0) as ctx:
            ctx.set_contacts(c)
            ctx.timing_reset()
            t = ctx.timing()
            assert all(v == dict(ms=0.0, launches=0, bytes=0.0) for v in t.values())
            ctx.row_sums()
            t, d = grown(ctx, t)
            assert d == {"row_sums": (1, 16.0 * sq)}
            ctx.row_sums()                                           # the sums are kept: no second pass
            t, d = grown(ctx, t)
            assert d == {}
            leaves, _z = ctx.upgma()
            st = ctx.nnchain_stats()
            t, d = grown(ctx, t)
            nn_launches, nn_bytes = d.pop("nnchain")
            assert nn_launches >= 1 and nn_bytes == _nnchain_bytes(n, st["scan_columns"])
            if presort:
                assert d == {"build_w": (1, 12.0 * sq), "presort_rows": (1, 10.0 * sq), "rank_invert": (1, 4.0 * sq)}
            else:
                assert d == {"build_w": (1, 12.0 * sq)}
            ctx.rank_matrix(leaves)
            t, d = grown(ctx, t)
            if presort:
                assert ctx.presort_state() == (1, 0)
                assert d == {"rank_relabel": (1, 4.0 * sq)}
            else:
                assert ctx.presort_state() == (0, 0)
                assert d == {"sort_rows": (1, 10.0 * sq), "rank_invert": (1, 4.0 * sq)}
            for start in (0, 777):
                m = n - start - 1
                ctx.cut_scan(start, n, .05)
                t, d = grown(ctx, t)
                flags = d.pop("hyper_flags")
                assert flags[0] == 1
                assert d == {"cut_count": (1, 2.0 * (m * (m + 3) / 2.0))}
                ctx.cut_scan(start, n // 2, .05)                     # S2C:473-477's rescan with another M: flags only
                t, d = grown(ctx, t)
                assert set(d) == {"hyper_flags"}
            sel = np.arange(300, 1501, dtype=np.int32)
            n2 = float(len(sel))
            ctx.p2_select(sel)
            t, d = grown(ctx, t)
            assert d == {"p2_select": (1, 16.0 * n2 * n2)}
            ctx.p2_total()
            t, d = grown(ctx, t)
            assert d == {"p2_total": (1, 4.0 * n2 * n2)}
            assert ctx.timing() == t


def test_timing_sums_the_part2_workers(hic, tmp_path, monkeypatch):
    """Part 2 with HICMI_PART2_WORKERS=3 (worker contexts: one per chromosome in the lock step, three threads):
    Context.timing() is the element-wise sum of _timing_one() over the context and its workers, the workers really did
    Part 2's launches, and timing_reset() zeroes them too."""
    from hic_genome_assembler_amd import orderGenome as p2
    monkeypatch.setattr(p2, "WORKERS", 3)
    lay, c = _synthetic(2100, 3)
    job = _Job(hic, c, lay, tmp_path)
    try:
        job.ctx.timing_enable(1)
        job.ctx.timing_reset()
        job.step()
        ctx = job.ctx
        assert len(ctx._workers) >= 3
        total = ctx.timing()
        parts = [ctx._timing_one()] + [w._timing_one() for w in ctx._workers]
        for k, v in total.items():
            assert v["launches"] == sum(p[k]["launches"] for p in parts), k
            assert v["bytes"] == sum(p[k]["bytes"] for p in parts), k
            expect_ms = parts[0][k]["ms"]
            for p in parts[1:]:
                expect_ms += p[k]["ms"]                                 # (the order Context.timing adds in)
            assert v["ms"] == expect_ms, k
        p2_families = [k for k in total if k.startswith("p2_")]
        assert sum(w._timing_one()[k]["launches"] for w in ctx._workers for k in p2_families) > 0
        assert all(p["nnchain"]["launches"] == 0 for p in parts[1:]) and parts[0]["nnchain"]["launches"] >= 1
        ctx.timing_reset()
        zero = dict(ms=0.0, launches=0, bytes=0.0)
        assert all(v == zero for v in ctx.timing().values())
        for w in ctx._workers:
            assert all(v == zero for v in w._timing_one().values())
        ctx.timing_enable(False)
    finally:
        job.close()


# The largest excess of sum(ms) over the host's interval that the unchanged library showed in five steps, measured before
# this test asserted anything ("Timing mode"): sum(ms) 15.4 - 15.7 ms in intervals of 29.4 - 30.2 ms, the
# largest excess -13.95 ms - no excess at all, so the measured slack of the two clocks is 0.  The allowance is twice that.
CLOCK_SLACK_MEASURED_MS = 0.0
CLOCK_SLACK_ALLOWED_MS = 2.0 * CLOCK_SLACK_MEASURED_MS


def test_summed_ms_fit_into_the_host_interval(hic, tmp_path, monkeypatch):
    """HICMI_NO_PRESORT=1 and one Part 2 worker: all work is on ONE in-order stream, so the timed regions cannot overlap, and
    between two synchronize() calls their sum cannot exceed the host's clock interval around them - the bound is 1.0 by
    construction, the only slack is the disagreement of the two clocks."""
    from hic_genome_assembler_amd import orderGenome as p2
    monkeypatch.setenv("HICMI_NO_PRESORT", "1")
    monkeypatch.setattr(p2, "WORKERS", 1)
    lay, c = _synthetic(2100, 3)
    job = _Job(hic, c, lay, tmp_path)
    try:
        job.step()                                                   # buffers, modules
        job.ctx.timing_enable(1)
        worst = -1e30
        for _ in range(5):
            job.ctx.timing_reset()
            job.ctx.synchronize()
            t0 = time.perf_counter()
            job.step()
            job.ctx.synchronize()
            host_ms = (time.perf_counter() - t0) * 1e3
            timing = job.ctx.timing()
            assert not job.ctx._workers
            total = sum(v["ms"] for v in timing.values())
            print("sum(ms) %.3f, host interval %.3f ms, excess %.3f" % (total, host_ms, total - host_ms))
            worst = max(worst, total - host_ms)
            assert total > 0.0 and timing["presort_rows"]["launches"] == 0
        print("largest excess of sum(ms) over the host interval: %.3f ms" % worst)
        assert worst <= CLOCK_SLACK_ALLOWED_MS
    finally:
        job.ctx.timing_enable(False)
        job.close()
