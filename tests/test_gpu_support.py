"""Placement support on the GPU (k_part2_support.hip through hicmi_p2_support_multi) against the CPU oracle's literal
cost of every candidate's explicit bin order (tests/support_reference.py).

Tolerances (fixed before any run): a score within 1e-10 relative of the oracle's - the project's bound for Part 2 scores
(tests/test_gpu_parity.py); a delta is the difference of two such scores: 2e-10 * score0 absolute; best_gap and
best_orientation EQUAL to the oracle's first strict maximum.  A verdict is compared wherever the oracle's deciding delta
is larger than that absolute bound (below it the sign of a difference of two fp64 scores is not defined)."""
import contextlib
import io
import os

import numpy as np
import pytest

import golden_cases as gc
import support_reference as ref

pytestmark = pytest.mark.gpu

REL = 1e-10
GOLDEN = [n for n in gc.case_names() if os.path.exists(os.path.join(gc.GOLDEN_DIR, n, "chromosomeOrders.txt"))]
# scaffolds / one-bin scaffolds / improvable rows of the golden orders, counted from the files with the oracle
COUNTS = {"n160": (30, 6, 0), "n600": (57, 3, 0), "n2000": (167, 16, 0)}


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    monkeypatch.delenv("HICMI_P2_SUPPORT_DIRECT", raising=False)


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _inputs(name, tmp_path):
    paths = _quiet(gc.write_case_files, name, str(tmp_path))
    files = {fn: os.path.join(gc.GOLDEN_DIR, name, fn) for fn in ("chromosomeGroups.txt", "chromosomeOrders.txt")}
    return paths, files["chromosomeGroups.txt"], files["chromosomeOrders.txt"]


def _support(paths, groups, orders, out):
    from hic_genome_assembler_amd import supportPart2 as sp
    return _quiet(sp.runSupport, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups, orders,
                  out)


def _compare(results, expected, label):
    """Every scored row of the table, score0, the deltas, the best moves and the verdicts against the oracle; prints the
    figures before asserting them."""
    worst, worst_delta, margin = 0.0, 0.0, np.inf
    problems = []
    for k, (got, exp) in enumerate(zip(results, expected)):
        assert got["names"] == exp["names"] and got["orientations"] == exp["orientations"]
        S = len(exp["names"])
        assert got["table"].shape == (S, S, 2)
        s0 = exp["score0"]
        if s0 != 0.0:
            worst = max(worst, abs(got["total"] - exp["total"]) / abs(exp["total"]), abs(got["score0"] - s0) / abs(s0))
        else:
            assert got["score0"] == 0.0 and got["total"] == exp["total"]
        bound = 2 * REL * abs(s0)
        for j, e in exp["rows"].items():
            g = got["rows"][j]
            t_got, t_exp = got["table"][j], exp["table"][j]
            if s0 != 0.0:
                worst = max(worst, float(np.max(np.abs(t_got - t_exp) / np.abs(t_exp))))
            else:
                assert not t_got.any()
            margin = min(margin, e.get("margin", np.inf) / abs(s0) if s0 else np.inf)
            if g["bins"] != e["bins"]:
                problems.append((k, j, "bins", g["bins"], e["bins"]))
            worst_delta = max(worst_delta, abs(g["flip_delta"] - e["flip_delta"]) / abs(s0) if s0 else 0.0)
            if e["bins"] == 1 and g["flip_delta"] != 0.0:
                problems.append((k, j, "one-bin flip_delta", g["flip_delta"], 0.0))
            if e["best"] is None:
                if not (g["best_gap"] is None and g["best_orientation"] is None and g["best_delta"] is None):
                    problems.append((k, j, "best", g["best_gap"], None))
            elif (g["best_gap"], g["best_orientation"]) != e["best"][:2]:
                problems.append((k, j, "best", (g["best_gap"], g["best_orientation"]), e["best"][:2]))
            else:
                worst_delta = max(worst_delta, abs(g["best_delta"] - e["best"][2]) / abs(s0))
            # the sign of a delta smaller than its bound is not defined: the verdict is compared everywhere else
            vague = (e["best"] is not None and abs(e["best"][2]) <= bound) or 0.0 < abs(e["flip_delta"]) <= bound
            if not vague and g["verdict"] != e["verdict"]:
                problems.append((k, j, "verdict", g["verdict"], e["verdict"]))
    print("%s: largest relative error of a score %.3e (bound %.0e), of a delta / score0 %.3e (bound %.0e), smallest "
          "relative margin of a best move %.3e" % (label, worst, REL, worst_delta, 2 * REL, margin))
    assert not problems, problems[:10]
    assert worst <= REL
    assert worst_delta <= 2 * REL


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_orders_against_the_oracle(name, tmp_path):
    paths, groups, orders = _inputs(name, tmp_path)
    results = _support(paths, groups, orders, str(tmp_path / "support.txt"))
    expected = _quiet(ref.reference_for_files, paths, groups, orders)
    rows = [r for x in expected for r in x["rows"].values()]
    counts = (len(rows), sum(r["bins"] == 1 for r in rows), sum(r["verdict"] == "improvable" for r in rows))
    print(name, "scaffolds / one-bin / improvable:", counts)
    if name in COUNTS:
        assert counts == COUNTS[name]
    _compare(results, expected, name)
    got_rows = [r for x in results for r in x["rows"]]
    assert sum(r["verdict"] == "improvable" for r in got_rows) == counts[2]
    assert sum(r["verdict"] == "orientation_open" for r in got_rows) == sum(r["verdict"] == "orientation_open" for r in rows)


@pytest.mark.parametrize("name", ["n600", "n2000"])
def test_default_path_against_direct(name, tmp_path, monkeypatch):
    paths, groups, orders = _inputs(name, tmp_path)
    a = _support(paths, groups, orders, str(tmp_path / "a.txt"))
    monkeypatch.setenv("HICMI_P2_SUPPORT_DIRECT", "1")
    b = _support(paths, groups, orders, str(tmp_path / "b.txt"))
    worst = 0.0
    for x, y in zip(a, b):
        assert x["score0"] == y["score0"] and x["total"] == y["total"]
        if y["score0"] != 0.0:
            worst = max(worst, float(np.max(np.abs(x["table"] - y["table"]) / np.abs(y["table"]))))
        for r, q in zip(x["rows"], y["rows"]):
            assert (r["best_gap"], r["best_orientation"], r["verdict"], r["bins"]) == \
                (q["best_gap"], q["best_orientation"], q["verdict"], q["bins"])
    print(name, "default against DIRECT: largest relative difference of a score %.3e" % worst)
    assert worst <= REL

    with open(str(tmp_path / "a.txt")) as fa, open(str(tmp_path / "b.txt")) as fb:
        assert fa.read() == fb.read()                         # the reported floats are literal scores on both paths


@pytest.mark.parametrize("name", ["n600", "n2000"])
def test_perturbed_orders_have_the_oracles_improvable_rows(name, tmp_path):
    paths, groups, orders = _inputs(name, tmp_path)
    g, o = ref.read_group_file(groups), ref.read_order_file(orders)
    c, a, b, f = ref.perturb(g, o)
    pert = str(tmp_path / "perturbed.txt")
    ref.write_order_file(pert, o)
    results = _support(paths, groups, pert, str(tmp_path / "support.txt"))
    expected = _quiet(ref.reference_for_files, paths, groups, pert)
    _compare(results, expected, name + " perturbed")
    want = [(j, e["best"][:2]) for j, e in expected[c]["rows"].items() if e["verdict"] == "improvable"]
    got = [(j, (r["best_gap"], r["best_orientation"])) for j, r in enumerate(results[c]["rows"]) if r["verdict"] == "improvable"]
    print(name, "perturbed chromosome", c + 1, "improvable rows:", want)
    assert got == want and len(want) >= 2
    assert results[c]["rows"][f]["flip_delta"] > 0 and expected[c]["rows"][f]["flip_delta"] > 0


def _decay_map(n, seed):
    rng = np.random.default_rng(seed)
    c = np.empty((n, n))
    idx = np.arange(n)
    for r0 in range(0, n, 1024):                              # slabs: no n x n temporaries besides the map itself
        r1 = min(n, r0 + 1024)
        d = np.abs(idx[r0:r1, None] - idx[None, :])
        c[r0:r1] = rng.uniform(0.5, 1.5, (r1 - r0, n)) * 100.0 / (1.0 + d) ** 1.1
    return np.ascontiguousarray(np.triu(c) + np.triu(c, 1).T)


def _explicit(host, groups, arrangements):
    from hic_genome_assembler_amd import orderGenome as p2
    from hic_genome_assembler_amd.hostio import Bin
    binList = [Bin(1000 + i, "c", i, i + 1, 1.0, 0.0) for i in range(len(host))]
    chromList = [sorted([binList[i].ID, name] for name, idx in g for i in idx) for g in groups]
    ordered = []
    for rows, arr in zip(chromList, arrangements):
        scaffs = []
        for name, o in arr:
            s = p2.Scaffold(name, sorted(b for b, x in rows if x == name), "+")
            if o == "-":
                s.flipOrientation()
            scaffs.append(s)
        ordered.append(scaffs)
    return binList, chromList, ordered


def _run_explicit(host, groups, arrangements, pick=None):
    """placementSupport on chromosomes given as [(scaffold, row indices)] lists and [(scaffold, orientation)]
    arrangements, and the oracle on the same."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    binList, chromList, ordered = _explicit(host, groups, arrangements)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(host)
        results = p2.placementSupport(p2.GenomeMatrix(ctx), ordered, binList, chromList)
    where = {b.ID: i for i, b in enumerate(binList)}
    expected = [ref.oracle_support(host, where, rows, arr, None if pick is None else pick(k, arr))
                for k, (rows, arr) in enumerate(zip(chromList, arrangements))]
    return results, expected


def _chromosome(prefix, first, lens):
    out, pos = [], first
    for i, ln in enumerate(lens):
        out.append(("%s%d" % (prefix, i), range(pos, pos + ln)))
        pos += ln
    return out, pos


def test_small_edges_in_one_call():
    """One scaffold; two; one-bin scaffolds only (every in-place flip ties); a single bin; scaffold and bin counts that
    are not multiples of 64 (67 scaffolds in 203 bins, 3 in 65) - all in one hicmi_p2_support_multi call."""
    rng = np.random.default_rng(11)
    groups, arrs, pos = [], [], 0
    for prefix, lens in (("solo", [37]), ("two", [5, 66]), ("ones", [1] * 9), ("bin", [1]),
                         ("odd", [int(v) for v in rng.integers(1, 6, 67)]), ("sixtyfive", [1, 63, 1])):
        g, pos = _chromosome(prefix, pos, lens)
        groups.append(g)
        order = rng.permutation(len(lens))
        arrs.append([(g[i][0], "-" if rng.random() < 0.5 else "+") for i in order])
    host = _decay_map(pos, 21)
    results, expected = _run_explicit(host, groups, arrs)
    _compare(results, expected, "edges")
    assert results[0]["rows"][0]["best_gap"] is None and results[0]["rows"][0]["verdict"] == "orientation_open"
    assert all(r["flip_delta"] == 0.0 and r["best_orientation"] == "+" for r in results[2]["rows"])
    assert results[3]["score0"] == 0.0 and results[3]["rows"][0]["best_gap"] is None
    from hic_genome_assembler_amd import orderGenome as p2
    assert p2.placementSupportText(results).count("\tNA\tNA\tNA\t") == 2


@pytest.mark.parametrize("kind", ["decay", "ones"])
def test_best_is_the_summary_of_the_devices_own_table(kind):
    """The device's pick against its host restatement on the SAME doubles: ``best`` of hicmi_p2_support_multi equals
    support_summary of the table that call returned - integer equality, no tolerance, both sides evaluate
    top - |top| * NEAR_TOP on the same numbers.  2 S candidates around the pick's 256-lane stride (S = 127, 128, 129) and
    its exits (S = 1: nothing competes; S = 2), scaffolds of 1 to 3 bins, one call.  On the map of ones many scores are
    exactly equal: the first of equals wins and near counts above 1 must occur."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    rng = np.random.default_rng(3)
    groups, arrs, pos = [], [], 0
    for S in (1, 2, 127, 128, 129):
        g, pos = _chromosome("s%d_" % S, pos, [int(v) for v in rng.integers(1, 4, S)])
        groups.append(g)
        arrs.append([(g[i][0], "-" if rng.random() < 0.5 else "+") for i in rng.permutation(S)])
    host = _decay_map(pos, 41) if kind == "decay" else np.ones((pos, pos))
    binList, chromList, ordered = _explicit(host, groups, arrs)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(host)
        matrix = p2.GenomeMatrix(ctx)
        matrix.bin_index(binList)
        (jobs,) = p2._layout_jobs(matrix.lanes(len(ordered)), ordered, binList, chromList)
        out = _lib.Context.p2_support_multi([(layout.ctx, ids, rev, total) for layout, ids, rev, total, _g in jobs])
    near = 0
    for (layout, ids, rev, _t, _g), (table, best) in zip(jobs, out):
        lengths = [layout.length[int(i)] for i in ids]
        assert table.shape == (len(ids), len(ids), 2) and (len(ids) == 1 or np.isfinite(table).all())
        assert np.array_equal(best, p2.support_summary(table, lengths, rev)), len(ids)
        near = max(near, int(best[:, 1].max()))
    print(kind, "map: largest near count", near)
    assert near > 1 or kind == "decay"


def test_a_chromosome_above_8192_bins_beside_a_small_one():
    """The mixed-size launch: 6 scaffolds in 8,300 bins and 5 scaffolds in 90 bins in one call (DESIGN.md 10 on dynamic
    LDS sized by a launch's largest chromosome); the oracle scores all 72 + 50 candidates."""
    big, pos = _chromosome("big", 0, [2100, 1, 1900, 1700, 1399, 1200])
    small, pos = _chromosome("small", pos, [40, 7, 1, 30, 12])
    arrs = [[("big3", "+"), ("big0", "-"), ("big1", "+"), ("big5", "-"), ("big2", "+"), ("big4", "-")],
            [("small2", "-"), ("small0", "+"), ("small4", "-"), ("small1", "+"), ("small3", "-")]]
    host = _decay_map(pos, 31)
    results, expected = _run_explicit(host, [big, small], arrs)
    assert expected[0]["n"] == 8300 > 8192
    _compare(results, expected, "8,300 bins beside 90")


SAMPLE = [0, 79, 7, 17, 31, 44, 58, 66]         # left-out scaffolds scored by the oracle (positions in the arrangement)


def test_bench_size_chromosome():
    """The smallest planted chromosome of bench.py's 16,000-bin map (seed 1): 1,026 bins in 80 scaffolds, in planted
    order and orientation.  The oracle scores all gaps of 8 left-out scaffolds fixed here (first, last, a one-bin one and
    five more); the rest of the table is held to the DIRECT path."""
    import torch
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(16000, seed=1)
    full = synth.dense_contacts_torch(lay, torch.device("cuda:0"), seed=1, sinkhorn_iters=12)
    chrom = int(lay.chrom_of_bin.max())
    rows = np.flatnonzero(lay.chrom_of_bin == chrom)
    host = np.ascontiguousarray(full[rows][:, rows].cpu().numpy())
    del full
    torch.cuda.empty_cache()
    scaf = lay.scaffold_of_bin[rows]
    ids = sorted(set(int(s) for s in scaf), key=lambda s: int(lay.scaffold_rank[s]))
    group = [(lay.scaffold_names[s], np.flatnonzero(scaf == s)) for s in sorted(ids)]
    arr = [(lay.scaffold_names[s], "+" if lay.scaffold_orient[s] > 0 else "-") for s in ids]
    lens = [int(np.count_nonzero(scaf == s)) for s in ids]
    print("bench-size chromosome: %d bins, %d scaffolds" % (len(rows), len(ids)))
    assert (len(rows), len(ids)) == (1026, 80)
    assert SAMPLE[0] == 0 and SAMPLE[1] == len(ids) - 1 and any(lens[j] == 1 for j in SAMPLE)
    results, expected = _run_explicit(host, [group], [arr], pick=lambda k, a: SAMPLE)
    _compare(results, expected, "bench-size chromosome, sampled")
    os.environ["HICMI_P2_SUPPORT_DIRECT"] = "1"
    try:
        direct, _e = _run_explicit(host, [group], [arr], pick=lambda k, a: [])
    finally:
        del os.environ["HICMI_P2_SUPPORT_DIRECT"]
    worst = float(np.max(np.abs(results[0]["table"] - direct[0]["table"]) / np.abs(direct[0]["table"])))
    print("bench-size chromosome: default against DIRECT, largest relative difference %.3e" % worst)
    assert worst <= REL
    assert [(r["best_gap"], r["best_orientation"], r["verdict"]) for r in results[0]["rows"]] == \
        [(r["best_gap"], r["best_orientation"], r["verdict"]) for r in direct[0]["rows"]]


def _config(tmp_path, paths, groups, n_scaffolds, scan_scaffolds, **extra):
    from hic_genome_assembler_amd import synth
    out = str(tmp_path / "out")
    cfg = synth.write_config(str(tmp_path / "config.txt"), paths, out, str(tmp_path / "plots"), 100000,
                             n_scaffolds=n_scaffolds, scan_scaffolds=scan_scaffolds)
    with open(os.path.join(out, "groups.txt"), "w") as fh, open(groups) as src:
        fh.write(src.read())
    with open(cfg, "a") as fh:                                # a later line replaces an earlier one
        fh.write("".join("%s = %s\n" % kv for kv in dict(extra, chromosomeGroupFile="groups.txt").items()))
    return cfg


def _shape(text):
    """A report without its floats: header prefixes, and per scaffold everything but the three float columns."""
    return [ln.split(" ### ")[0] if ln.startswith("#") else ln.split("\t")[:3] + ln.split("\t")[4:6] + ln.split("\t")[7:]
            for ln in text.splitlines()]


def test_command_lines_write_the_same_report(tmp_path):
    """supportPart2 on the reference-written order file of n2000, -part2 with placementSupportFile (which reproduces that
    order file) and sweepPart2 -support at the one setting."""
    from hic_genome_assembler_amd import run_hicAssembler as run, supportPart2 as sp, sweepPart2 as sw
    name = "n2000"
    spec = gc.load_case(name)[0]
    paths, groups, orders = _inputs(name, tmp_path)
    cfg = _config(tmp_path, paths, groups, spec["n_scaffolds"], spec["scan_scaffolds"],
                  placementSupportFile="support_part2.txt")
    out = str(tmp_path / "out")
    _quiet(sp.main, ["-config", cfg, "-chromosomeOrderFile", orders, "-out", os.path.join(out, "support_cli.txt")])
    _quiet(run.main, ["-part2", "-config", cfg])
    v = run.readConfigFileToVariables(cfg)
    with open(v["chromosomeOrderFile"]) as fh:
        assert fh.read() == gc.golden_text(name, "chromosomeOrders.txt")
    with open(os.path.join(out, "support_cli.txt")) as a, open(os.path.join(out, "support_part2.txt")) as b:
        report = a.read()
        assert report == b.read()
    expected = _quiet(ref.reference_for_files, paths, groups, orders)
    assert _shape(report) == _shape(ref.report_text(expected))
    _quiet(sw.main, ["-config", cfg, "-out", os.path.join(out, "sweep"), "-support"])
    with open(os.path.join(out, "sweep", "best", "placementSupport.txt")) as fh:
        assert fh.read() == report
    with open(os.path.join(out, "sweep", "best", os.path.basename(v["chromosomeOrderFile"]))) as fh:
        assert fh.read() == gc.golden_text(name, "chromosomeOrders.txt")
    # score0 is the sweep's final_score: the same literal objective under the same total
    with open(os.path.join(out, "sweep", "chromosome_scores.tsv")) as fh:
        final_scores = [ln.split("\t")[3] for ln in fh.read().splitlines()[1:]]
    assert final_scores == [ln.split(" ### ")[1] for ln in report.splitlines() if ln.startswith("#")]
