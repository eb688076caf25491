"""Wide Part 2 windows decided from a device short list, and the Part 2 sweep, on the GPU.

* hicmi_p2_window_shortlist returns, for k = 2 ... 8, the same index lists and bit-identical fast scores as a NumPy
  restatement of api.hip's short_list over hicmi_p2_score_window's deltas (several windows and floors, a quantised map
  with exact zeros, one-bin scaffolds, an overflow);
* the device path changes no ordering: HICMI_P2_DEVICE_DECIDE=2 against off on the goldens and planted chromosomes;
* 8-wide brute force and scan windows against a test-local restatement scored by the CPU oracle;
* sweepPart2 against separate -part2 runs, setting by setting.
"""
import contextlib
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR_TOP = 1e-9


def _contacts(lay, seed, quantise=None):
    from hic_genome_assembler_amd import synth
    c = synth.dense_contacts(lay, seed=seed, sinkhorn_iters=8)
    if quantise is not None:
        frac, decimals = quantise
        c = np.round(c, decimals)
        c[c <= np.quantile(c, frac)] = 0.0
        c = 0.5 * (c + c.T)
        np.fill_diagonal(c, np.maximum(np.diag(c), 1.0))
    return np.ascontiguousarray(c)


def host_short_list(delta, whole, total, cur_fast, c0, floor):
    """api.hip's short_list over decide_from_delta's fast scores."""
    fast = delta / total if whole else cur_fast + (delta - delta[c0]) / total
    ok = np.isfinite(fast)
    if not ok.any():
        return np.zeros(0, np.int64), np.zeros(0)
    mx = float(fast[ok].max())
    top = mx if mx > floor else floor
    thr = top - abs(top) * NEAR_TOP
    near = np.flatnonzero(ok & (fast >= thr))
    return near, fast[near]


def _chromosome_ctx(ctx, c, lens, rev):
    """One chromosome of scaffolds with ``lens`` bins (consecutive bins of ``c``) in that order and orientation."""
    ctx.set_contacts(c)
    n = int(sum(lens))
    ctx.p2_select(np.arange(n, dtype=np.int32))
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    ctx.p2_layout(starts, np.asarray(lens, np.int32))
    ids = np.arange(len(lens), dtype=np.int32)
    ctx.p2_set_arrangement(ids, np.asarray(rev, np.uint8))
    return ids


def _check_windows(ctx, k, S, rev, first, count, floors, cap=4096):
    from hic_genome_assembler_amd import orderGenome as p2
    orders, orients = p2._enumeration(k)
    ctx.p2_window_tables(np.asarray(orders, np.int8),
                         np.asarray([[1 if sg == "-" else 0 for sg in r] for r in orients], np.uint8))
    total = ctx.p2_arrangement_total()
    whole = k == S
    cur_fast = 0.0 if whole else ctx.p2_arrangement_score(total)
    checked = 0
    for floor in floors(cur_fast):
        got = ctx.p2_window_shortlist(first, count, k, total, floor, None if whole else cur_fast, cap)
        for w in range(count):
            delta = ctx.p2_score_window(first + w, k)
            c0 = p2._orient_index(k, ["-" if r else "+" for r in rev[first + w:first + w + k]])
            near, fast = host_short_list(delta, whole, total, cur_fast, c0, floor)
            if len(near) > cap:
                assert got[w] is None, (k, w, floor)
                continue
            assert got[w] is not None, (k, w, floor)
            assert np.array_equal(got[w][0], near), (k, w, floor)
            assert got[w][1].tobytes() == fast.tobytes(), (k, w, floor)
            checked += 1
    return checked


def _floors(delta_hi):
    return lambda cur: [0.0, cur, cur + delta_hi]


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7, 8])
def test_shortlist_equals_host_list(k):
    from hic_genome_assembler_amd import _lib, synth
    lay = synth.make_layout(260, seed=40 + k, n_chrom=1, mean_scaffold_bins=9.0)
    c = _contacts(lay, 40 + k)
    rng = np.random.default_rng(k)
    lens = [int(v) for v in rng.integers(1, 25, size=k + 3)]
    rev = rng.integers(0, 2, size=len(lens)).astype(np.uint8)
    with _lib.Context(0) as ctx:
        _chromosome_ctx(ctx, c, lens, rev)
        count = 2 if k == 8 else 4
        assert _check_windows(ctx, k, len(lens), rev, 0, count, _floors(1.0)) > 0
        # k == S: the brute-force form (fast = delta / total)
        _chromosome_ctx(ctx, c, lens[:k], rev[:k])
        assert _check_windows(ctx, k, k, rev[:k], 0, 1, _floors(1.0)) > 0


@pytest.mark.parametrize("k", [5, 7, 8])
def test_shortlist_quantised_and_one_bin_scaffolds(k):
    """Exact zeros and equal values (ties between fast scores), windows of one-bin scaffolds (orientation ties: every
    flip of a one-bin scaffold is the same bin order), and a list that overflows a small cap."""
    from hic_genome_assembler_amd import _lib, synth
    lay = synth.make_layout(200, seed=7 + k, n_chrom=1, mean_scaffold_bins=4.0)
    c = _contacts(lay, 7 + k, quantise=(0.4, 2))
    lens = [3, 1, 1, 2, 1, 1, 1, 1, 4, 1, 1]
    rev = np.array([0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1], np.uint8)
    with _lib.Context(0) as ctx:
        _chromosome_ctx(ctx, c, lens, rev)
        assert _check_windows(ctx, k, len(lens), rev, 1, 2, _floors(0.0)) > 0
        # one-bin scaffolds only: 2^k orientations of each order give one bin order, so the near-top list is >= 2^k long
        ones = [1] * (k + 2)
        rev1 = np.zeros(len(ones), np.uint8)
        _chromosome_ctx(ctx, c, ones, rev1)
        assert _check_windows(ctx, k, len(ones), rev1, 0, 3, lambda cur: [0.0, cur]) > 0
        got = ctx.p2_window_shortlist(0, 3, k, ctx.p2_arrangement_total(), 0.0, None, 4)
        assert all(g is None for g in got)                  # > 4 candidates tie at the top: every window overflows
        assert _check_windows(ctx, k, len(ones), rev1, 0, 3, lambda cur: [0.0], cap=4) == 0


def _groups_file(path, lay, chroms=None):
    with open(path, "w") as fh:
        for g in (range(int(lay.chrom_of_bin.max()) + 1) if chroms is None else chroms):
            fh.write("### Chromosome group %d ###\n" % (g + 1))
            for k in np.flatnonzero(lay.chrom_of_bin == g):
                fh.write("%d\t%s\n" % (lay.bin_ids[k], lay.scaffold_names[lay.scaffold_of_bin[k]]))
    return str(path)


def _part2_files(paths, groups, out, nS, sc):
    from hic_genome_assembler_amd import orderGenome as p2
    os.makedirs(out, exist_ok=True)
    f = lambda k: os.path.join(out, k)  # noqa: E731
    p2.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups,
                   f("chromosomeOrders.txt"), False, False, False, "t", f("plotOrder.txt"), nS, sc, 100000)
    return {k: open(f(k)).read() for k in ("chromosomeOrders.txt", "plotOrder.txt")}


DEVICE_CASES = [
    # name, bins, chromosomes, mean scaffold bins, quantise, nScaffolds, scanScaffolds
    ("bench-scaffolds-1800", 1800, 4, 13.0, None, 6, 5),
    ("quantised-900", 900, 3, 6.0, (0.3, 2), 6, 5),
    ("one-bin-scaffolds", 260, 3, 1.6, None, 6, 5),
    ("two-scaffold-windows", 180, 2, 6.0, None, 3, 2),
]


@pytest.mark.parametrize("case", ["n160", "n400_default", "n600"] + [c[0] for c in DEVICE_CASES])
def test_device_decisions_change_nothing(case, tmp_path, monkeypatch):
    """Every window of >= 2 scaffolds through the device short list against every window through the downloaded deltas:
    identical files (and the reference-written ones where a fixture exists)."""
    import golden_cases as gc
    from hic_genome_assembler_amd import synth
    gold = None
    if case.startswith("n"):
        spec = gc.load_case(case)[0]
        paths = gc.write_case_files(case, str(tmp_path))
        groups = str(tmp_path / "groups.txt")
        with open(groups, "w") as fh:
            fh.write(gc.golden_text(case, "chromosomeGroups.txt"))
        nS, sc = spec["n_scaffolds"], spec["scan_scaffolds"]
        gold = {k: gc.golden_text(case, k) for k in ("chromosomeOrders.txt", "plotOrder.txt")}
    else:
        _name, n, n_chrom, mean, quantise, nS, sc = next(c for c in DEVICE_CASES if c[0] == case)
        lay = synth.make_layout(n, seed=300 + n, n_chrom=n_chrom, mean_scaffold_bins=mean)
        paths = synth.write_hicpro(str(tmp_path / "in"), lay, _contacts(lay, 300 + n, quantise), "d")
        groups = _groups_file(tmp_path / "groups.txt", lay)
    outs = {}
    for mode in ("2", "off"):
        monkeypatch.setenv("HICMI_P2_DEVICE_DECIDE", mode)
        outs[mode] = _part2_files(paths, groups, str(tmp_path / mode), nS, sc)
    assert outs["2"] == outs["off"]
    if gold is not None:
        assert outs["2"] == gold


def test_seven_wide_windows_against_the_oracle(tmp_path):
    """7 / 7 and 7 / 6 end to end against Part2Oracle on one chromosome of 8 small scaffolds."""
    import time

    import hic_oracle as orc
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(120, seed=77, n_chrom=3, mean_scaffold_bins=4.0)
    c = _contacts(lay, 77)
    paths = synth.write_hicpro(str(tmp_path / "in"), lay, c, "d")
    counts = [len(set(lay.scaffold_of_bin[lay.chrom_of_bin == g])) for g in range(3)]
    g = int(np.argmin([abs(v - 8) for v in counts]))
    groups = _groups_file(tmp_path / "groups.txt", lay, [g])
    t_oracle = 0.0
    for nS, sc in ((7, 7), (7, 6)):
        got = _part2_files(paths, groups, str(tmp_path / ("gpu%d%d" % (nS, sc))), nS, sc)
        ref = tmp_path / ("orc%d%d" % (nS, sc))
        ref.mkdir()
        t = time.time()
        orc.run_part2(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups,
                      str(ref / "chromosomeOrders.txt"), str(ref / "plotOrder.txt"), n_scaffolds=nS, scan_scaffolds=sc,
                      batch=True)
        t_oracle += time.time() - t
        for k in ("chromosomeOrders.txt", "plotOrder.txt"):
            assert got[k] == (ref / k).read_text(), (nS, sc, k)
    print("oracle: %.1f s for 7/7 and 7/6 on %d scaffolds" % (t_oracle, counts[g]))


def _candidate_rows(pieces, orders, orients):
    """Bin rows of every candidate of a window (order-major, orientations inner): pieces[j] = (forward, reversed)."""
    sign = np.array([[1 if s == "-" else 0 for s in r] for r in orients], bool)
    for o in orders:
        cols = [np.where(sign[:, s:s + 1], pieces[j][1][None, :], pieces[j][0][None, :]) for s, j in enumerate(o)]
        yield np.concatenate(cols, axis=1)


def _first_strict_max(mat, head, tail, pieces, orders, orients, total, floor):
    import hic_oracle as orc
    best, pick, base = floor, -1, 0
    chunk = []
    n_ori = len(orients)

    def flush(chunk, base):
        nonlocal best, pick
        rows = np.concatenate(chunk, axis=0)
        rows = np.concatenate([np.broadcast_to(head, (len(rows), len(head))), rows,
                               np.broadcast_to(tail, (len(rows), len(tail)))], axis=1).astype(np.int32)
        vals = orc.cost_literal_rows(mat, np.ascontiguousarray(rows), total)
        i = int(np.argmax(vals))                            # the first of the chunk's maxima: where `v > best` stops
        if vals[i] > best:
            best, pick = float(vals[i]), base + i
    for rows in _candidate_rows(pieces, orders, orients):
        chunk.append(rows)
        if len(chunk) == 400:
            flush(chunk, base)
            base += 400 * n_ori
            chunk = []
    if chunk:
        flush(chunk, base)
    return pick, best


@pytest.mark.parametrize("k", [8, 7])
def test_eight_wide_brute_force_and_scan_round(k):
    """nScaffolds 8: the brute force over 8 scaffolds (5,160,960 candidates) and one scan round of k-wide windows
    against a restatement that scores every candidate literally and takes the first strict maximum."""
    import hic_oracle as orc
    from hic_genome_assembler_amd import _lib, orderGenome as p2, synth
    lay = synth.make_layout(200, seed=88, n_chrom=1, mean_scaffold_bins=6.0)
    c = _contacts(lay, 88)
    lens = [4, 3, 3, 2, 2, 2, 2, 2, 2]
    n = sum(lens)
    mat = np.ascontiguousarray(c[:n, :n])
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    pieces = [(np.arange(s, s + L, dtype=np.int32), np.arange(s + L - 1, s - 1, -1, dtype=np.int32))
              for s, L in zip(starts, lens)]
    orders8, orients8 = p2._enumeration(8)
    with _lib.Context(0) as ctx:
        rev = np.zeros(len(lens), np.uint8)
        _chromosome_ctx(ctx, c, lens, rev)
        # brute force: the 8 largest scaffolds alone (k == S)
        ctx.p2_set_arrangement(np.arange(8, dtype=np.int32), rev[:8])
        ctx.p2_window_tables(np.asarray(orders8, np.int8),
                             np.asarray([[1 if s == "-" else 0 for s in r] for r in orients8], np.uint8))
        total = ctx.p2_arrangement_total()
        pick, best, _pf = ctx.p2_decide_window(0, 8, total, 0.0, None)
        e = np.zeros(0, np.int32)
        want = _first_strict_max(mat, e, e, pieces[:8], orders8, orients8, total, 0.0)
        assert (pick, best) == want
        # one scan round over all 9 scaffolds, windows of k, from the brute force's arrangement + the 9th scaffold
        o, r = orders8[pick // len(orients8)], orients8[pick % len(orients8)]
        ids = [int(j) for j in o] + [8]
        rv = [1 if s == "-" else 0 for s in r] + [0]
        ctx.p2_set_arrangement(np.asarray(ids, np.int32), np.asarray(rv, np.uint8))
        total = ctx.p2_arrangement_total()
        row = np.concatenate([pieces[i][v] for i, v in zip(ids, rv)])
        floor = float(orc.cost_literal_rows(mat, row[None, :].astype(np.int32), total)[0]) * (1 - 1e-6)
        orders, orients = p2._enumeration(k)
        ctx.p2_window_tables(np.asarray(orders, np.int8),
                             np.asarray([[1 if s == "-" else 0 for s in x] for x in orients], np.uint8))
        g_ids, g_rev, g_best, _cf, g_imp = ctx.p2_scan_pass(ids, rv, k, total, floor, None)
        best, w_ids, w_rev, improved = floor, list(ids), list(rv), False
        for first in range(len(ids) - k + 1):
            head = np.concatenate([pieces[i][v] for i, v in zip(w_ids[:first], w_rev[:first])] + [e])
            tail = np.concatenate([pieces[i][v] for i, v in zip(w_ids[first + k:], w_rev[first + k:])] + [e])
            win = w_ids[first:first + k]
            p, b = _first_strict_max(mat, head, tail, [pieces[i] for i in win], orders, orients, total, best)
            if p >= 0:
                o, r = orders[p // len(orients)], orients[p % len(orients)]
                w_ids[first:first + k] = [win[j] for j in o]
                w_rev[first:first + k] = [1 if s == "-" else 0 for s in r]
                best, improved = b, True
        assert [int(v) for v in g_ids] == w_ids and [int(v) for v in g_rev] == w_rev
        assert g_best == best and g_imp == improved


SWEEP_MAPS = ["n400_default", "synthetic-1800"]


@pytest.mark.parametrize("case", SWEEP_MAPS)
def test_sweep_equals_separate_runs(case, tmp_path, monkeypatch):
    """Grid {4,6,8} x {3,5,8}: every setting's files equal run_hicAssembler -part2 at that setting, part2.log a one-worker
    run's lines; the planner shares brute force and insertion; best/ takes each chromosome from its argmax setting; every
    final_score is the oracle's literal score of the written bin order under the chromosome's selection total."""
    import golden_cases as gc
    import hic_oracle as orc
    from test_sweep_part2_cpu import _config, part2_log
    from hic_genome_assembler_amd import _lib, orderGenome as p2, run_hicAssembler as run, sweepPart2 as sw, synth
    if case.startswith("n"):
        _spec, _meta, _gold, lay, c = gc.load_case(case)
        paths = gc.write_case_files(case, str(tmp_path))
        groups = str(tmp_path / "groups.txt")
        with open(groups, "w") as fh:
            fh.write(gc.golden_text(case, "chromosomeGroups.txt"))
    else:
        lay = synth.make_layout(1800, seed=18, n_chrom=4, mean_scaffold_bins=13.0)
        c = _contacts(lay, 18)
        paths = synth.write_hicpro(str(tmp_path / "in"), lay, c, "d")
        groups = _groups_file(tmp_path / "groups.txt", lay)
    out = tmp_path / "sweep"
    with contextlib.redirect_stdout(io.StringIO()):
        res = sw.runSweep(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups,
                          "chromosomeOrders.txt", "plotOrder.txt", [4, 6, 8], [3, 5, 8], str(out))
    grid = res["grid"]
    n_chrom = len(res["orders"][0])
    assert grid == [(4, 3), (4, 4), (6, 3), (6, 5), (6, 6), (8, 3), (8, 5), (8, 8)]
    assert res["counts"]["start_jobs"] < len(grid) * n_chrom
    assert len(set(res["scan_keys"])) == len(res["scan_keys"]) == res["counts"]["scan_jobs"]
    for g in grid:
        d = out / sw.setting_name(*g)
        (tmp_path / ("run%d%d" % g)).mkdir()
        cfg = _config(tmp_path / ("run%d%d" % g), paths, "chromosomeGroups.txt", nScaffolds=str(g[0]),
                      scanScaffolds=str(g[1]))
        saved = tmp_path / ("run%d%d" % g) / "files"
        (saved / "chromosomeGroups.txt").write_text(open(groups).read())
        with contextlib.redirect_stdout(io.StringIO()):
            run.main(["-part2", "-config", cfg])
        for f in ("chromosomeOrders.txt", "plotOrder.txt"):
            assert (d / f).read_text() == (saved / f).read_text(), (g, f)
        monkeypatch.setattr(p2, "WORKERS", 1)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            run.main(["-part2", "-config", cfg])
        monkeypatch.undo()
        assert (d / "part2.log").read_text().splitlines() == part2_log(buf.getvalue()), g
    # best/ and final_score
    rows = sw.read_summary(str(out / "sweep_summary.tsv"))
    best = res["best"]
    chunks = (out / "best" / "chromosomeOrders.txt").read_text().split("### Chromosome grouping ")[1:]
    assert len(chunks) == n_chrom
    for ci in range(n_chrom):
        scores = [r["final_scores"][ci] for r in rows]
        assert best[ci] == scores.index(max(scores))
        want = (out / sw.setting_name(*grid[best[ci]]) / "chromosomeOrders.txt").read_text()
        assert chunks[ci] == want.split("### Chromosome grouping ")[ci + 1]
    where = {int(b): i for i, b in enumerate(lay.bin_ids)}
    group_lines = [ln for ln in open(groups).read().split("\n")[1:]]
    chroms, cur = [], []
    for ln in group_lines:
        if ln.startswith("#"):
            chroms.append(cur)
            cur = []
        elif ln:
            cur.append((int(ln.split("\t")[0]), ln.split("\t")[1]))
    chroms.append(cur)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(c)
        for ci, chrom in enumerate(chroms):
            scaffs, _d = p2.initiateBinsAndScaffolds(chrom)
            ctx.p2_select(np.asarray([where[b] for s in scaffs for b in sorted(s.binList)], np.int32))
            total = ctx.p2_total()
            for si, g in enumerate(grid):
                order = [where[b] for s in res["orders"][si][ci] for b in s.binList]
                lit = orc.cost_literal_rows(c, np.asarray([order], np.int32), total)[0]
                assert rows[si]["final_scores"][ci] == res["scores"][si][ci] == float(lit), (g, ci)


def test_sweep_takes_the_batched_calls(tmp_path, monkeypatch):
    """The sweep runs on the driver of a -part2 run, so on a real context it reaches hicmi_p2_start_all and
    hicmi_p2_scan_arranged; with both switched off it reaches neither and writes the same tree, file for file."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2, sweepPart2 as sw, synth
    lay = synth.make_layout(1800, seed=18, n_chrom=4, mean_scaffold_bins=13.0)
    paths = synth.write_hicpro(str(tmp_path / "in"), lay, _contacts(lay, 18), "d")
    groups = _groups_file(tmp_path / "groups.txt", lay)
    calls = []
    start_all, scan_arranged = _lib.Context.p2_start_all, _lib.Context.p2_scan_arranged
    monkeypatch.setattr(_lib.Context, "p2_start_all",
                        staticmethod(lambda jobs, tables: (calls.append("start_all"), start_all(jobs, tables))[1]))
    monkeypatch.setattr(_lib.Context, "p2_scan_arranged",
                        lambda self, *a: (calls.append("scan_arranged"), scan_arranged(self, *a))[1])
    trees = {}
    for batched in (True, False):
        monkeypatch.setattr(p2, "START_ALL", batched)
        monkeypatch.setattr(p2, "SCAN_ARRANGED", batched)
        del calls[:]
        out = tmp_path / ("sweep%d" % batched)
        with contextlib.redirect_stdout(io.StringIO()):
            res = sw.runSweep(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups,
                              "chromosomeOrders.txt", "plotOrder.txt", [4, 6], [3, 5], str(out))
        assert res["grid"] == [(4, 3), (4, 4), (6, 3), (6, 5)]
        if batched:
            assert calls.count("start_all") == 1                 # every start job of the sweep in the one call
            assert calls.count("scan_arranged") == sum(1 for fk in res["scan_keys"] if fk[2] is not None) > 0
        else:
            assert calls == []
        trees[batched] = {os.path.relpath(os.path.join(d, f), str(out)): open(os.path.join(d, f)).read()
                          for d, _dirs, files in os.walk(str(out)) for f in files}
    assert sorted(trees[True]) == sorted(trees[False]) and len(trees[True]) == 3 * 4 + 2 + 2
    for name in trees[True]:
        assert trees[True][name] == trees[False][name], name
