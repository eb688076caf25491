"""Break support on the GPU (k_part2_breaks.hip through hicmi_p2_breaks_multi) against the CPU oracle's literal cost of
every candidate's explicit bin order (tests/break_reference.py).

Tolerances (fixed before any run, those of tests/test_gpu_support.py): a score within 1e-10 relative of the oracle's; a
delta is the difference of two such scores: 2e-10 * |score0| absolute; the best (cut, move) EQUAL to the oracle's first
strict maximum.  A verdict is compared wherever the oracle's |best_delta| is larger than that absolute bound (below it
the sign of a difference of two fp64 scores is not defined)."""
import contextlib
import io
import os

import numpy as np
import pytest

import break_reference as ref
import golden_cases as gc
from support_reference import read_group_file, read_order_file, write_order_file

pytestmark = pytest.mark.gpu

REL = 1e-10
GOLDEN = [n for n in gc.case_names() if os.path.exists(os.path.join(gc.GOLDEN_DIR, n, "chromosomeOrders.txt"))]
# multi-bin scaffolds / NA rows among them (two bins) / breakable rows of the golden orders, counted from the text files
# with the oracle
COUNTS = {"n160": (24, 4, 1), "n160_numba": (24, 4, 1), "n300_edges": (35, 4, 1), "n400_default": (42, 4, 4),
          "n600": (54, 6, 2), "n2000": (151, 14, 5), "n500_sparse": (54, 8, 0)}


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    monkeypatch.delenv("HICMI_P2_BREAKS_DIRECT", raising=False)


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _inputs(name, tmp_path):
    paths = _quiet(gc.write_case_files, name, str(tmp_path))
    files = {fn: os.path.join(gc.GOLDEN_DIR, name, fn) for fn in ("chromosomeGroups.txt", "chromosomeOrders.txt")}
    return paths, files["chromosomeGroups.txt"], files["chromosomeOrders.txt"]


def _breaks(paths, groups, orders, out, **kw):
    from hic_genome_assembler_amd import supportBreaks as sb
    return _quiet(sb.runBreaks, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups, orders,
                  out, **kw)


def _compare(results, expected, label):
    """Every scored cut of the tables, score0, the best breaks, their deltas and the verdicts against the oracle; prints
    the figures before asserting them."""
    worst, worst_delta, margin, gain = 0.0, 0.0, np.inf, np.inf
    problems = []
    for k, (got, exp) in enumerate(zip(results, expected)):
        assert got["names"] == exp["names"] and got["orientations"] == exp["orientations"]
        s0 = exp["score0"]
        if s0 != 0.0:
            worst = max(worst, abs(got["total"] - exp["total"]) / abs(exp["total"]), abs(got["score0"] - s0) / abs(s0))
        else:
            assert got["score0"] == 0.0 and got["total"] == exp["total"]
        bound = 2 * REL * abs(s0)
        assert len(got["table"]) == sum(len(b) for b in exp["blocks"])
        for j, e in exp["rows"].items():
            g = got["rows"][j]
            t_exp = exp["blocks"][j]
            t_got = got["table"][got["offsets"][j]:got["offsets"][j] + len(t_exp)]
            assert t_got.shape == t_exp.shape == (max(e["bins"] - 1, 0), 8)
            scored = ~np.isnan(t_exp)
            if s0 != 0.0 and scored.any():
                worst = max(worst, float(np.max(np.abs(t_got[scored] - t_exp[scored]) / np.abs(t_exp[scored]))))
            elif s0 == 0.0:
                assert not t_got.any()
            if g["bins"] != e["bins"]:
                problems.append((k, j, "bins", g["bins"], e["bins"]))
            if e.get("sampled"):
                continue
            if e["best"] is None:
                if not (g["best_cut"] is None and g["cut_after_bin"] is None and g["best_move"] is None
                        and g["best_delta"] is None and g["gain"] is None and g["verdict"] == "NA"):
                    problems.append((k, j, "best", g["best_cut"], None))
                continue
            margin, gain = min(margin, e["margin"] / abs(s0)), min(gain, abs(e["gain"]))
            if (g["best_cut"], g["cut_after_bin"], g["best_move"]) != (e["cut"], e["after"], e["move"]):
                problems.append((k, j, "best", (g["best_cut"], g["cut_after_bin"], g["best_move"]), (e["cut"], e["after"], e["move"])))
                continue
            worst_delta = max(worst_delta, abs(g["best_delta"] - e["delta"]) / abs(s0))
            # the sign of a delta smaller than its bound is not defined: the verdict is compared everywhere else
            if abs(e["delta"]) > bound and g["verdict"] != e["verdict"]:
                problems.append((k, j, "verdict", g["verdict"], e["verdict"]))
    print("%s: largest relative error of a score %.3e (bound %.0e), of a delta / score0 %.3e (bound %.0e), smallest |gain| "
          "%.3e, smallest relative margin of a best break over its runner-up %.3e" % (label, worst, REL, worst_delta, 2 * REL,
                                                                                      gain, margin))
    assert not problems, problems[:10]
    assert worst <= REL
    assert worst_delta <= 2 * REL
    return gain


def _shape(text):
    """A report without its floats: header prefixes, and per scaffold everything but best_delta and gain."""
    return [ln.split(" ### ")[0] if ln.startswith("#") else ln.split("\t")[:6] + ln.split("\t")[8:] for ln in text.splitlines()]


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_orders_against_the_oracle(name, tmp_path):
    paths, groups, orders = _inputs(name, tmp_path)
    results = _breaks(paths, groups, orders, str(tmp_path / "breaks.txt"), brokenFile=str(tmp_path / "broken.txt"))
    expected = _quiet(ref.reference_for_files, paths, groups, orders)
    rows = [r for x in expected for r in x["rows"].values()]
    counts = (sum(r["bins"] > 1 for r in rows), sum(r["bins"] > 1 and r["verdict"] == "NA" for r in rows),
              sum(r["verdict"] == "breakable" for r in rows))
    print(name, "multi-bin scaffolds / NA among them / breakable:", counts)
    assert counts == COUNTS[name]
    gain = _compare(results, expected, name)
    assert gain > 2 * REL                                     # no golden row's verdict is left uncompared
    got_rows = [r for x in results for r in x["rows"]]
    for verdict in ("breakable", "intact", "NA"):
        assert sum(r["verdict"] == verdict for r in got_rows) == sum(r["verdict"] == verdict for r in rows)
    with open(str(tmp_path / "breaks.txt")) as fh:
        report = fh.read().splitlines()
    assert _shape("\n".join(report)) == _shape(ref.report_text(expected))
    with open(str(tmp_path / "broken.txt")) as fh:
        assert fh.read() == ref.broken_text(expected, gc.golden_text(name, "chromosomeGroups.txt"))


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


@pytest.mark.parametrize("name", ["n600", "n2000"])
def test_planted_misjoins_are_found_at_the_junction(name, tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run
    paths, groups, orders = _inputs(name, tmp_path)
    g2, o2, c, i, joined, junction = ref.plant_misjoin(read_group_file(groups), read_order_file(orders))
    groups2, orders2, broken = str(tmp_path / "groups2.txt"), str(tmp_path / "orders2.txt"), str(tmp_path / "broken.txt")
    ref.write_group_file(groups2, g2)
    write_order_file(orders2, o2)
    results = _breaks(paths, groups2, orders2, str(tmp_path / "breaks.txt"), brokenFile=broken)
    expected = _quiet(ref.reference_for_files, paths, groups2, orders2)
    _compare(results, expected, name + " with a planted misjoin")
    row, want = results[c]["rows"][i], expected[c]["rows"][i]
    print(name, "planted: chromosome %d, %s, junction after %d of %d bins; best_cut %s, %s, gain %r (oracle: %s, %s, %r)"
          % (c + 1, joined, junction, row["bins"], row["best_cut"], row["best_move"], row["gain"], want["cut"], want["move"],
             want["gain"]))
    assert results[c]["names"][i] == joined
    assert want["verdict"] == "breakable" and want["cut"] == junction
    assert row["verdict"] == "breakable" and row["best_cut"] == junction
    with open(groups2) as fh:
        group_text = fh.read()
    with open(broken) as fh:
        assert fh.read() == ref.broken_text(expected, group_text)
    # -part2 on the broken file orders the two pieces as scaffolds of their own
    spec = gc.load_case(name)[0]
    cfg = _config(tmp_path, paths, broken, spec["n_scaffolds"], spec["scan_scaffolds"])
    _quiet(run.main, ["-part2", "-config", cfg])
    listed = [a for chrom in read_order_file(run.readConfigFileToVariables(cfg)["chromosomeOrderFile"]) for a, _o in chrom]
    assert joined + ".brk1" in listed and joined + ".brk2" in listed and joined not in listed


def _decay_map(n, seed):
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    c = rng.uniform(0.5, 1.5, (n, n)) * 100.0 / (1.0 + np.abs(idx[:, None] - idx[None, :])) ** 1.1
    return np.ascontiguousarray(np.triu(c) + np.triu(c, 1).T)


def _chromosome(prefix, first, lens):
    out, pos = [], first
    for i, ln in enumerate(lens):
        out.append(("%s%d" % (prefix, i), range(pos, pos + ln)))
        pos += ln
    return out, pos


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


def _run_explicit(host, groups, arrangements, min_piece=1, cuts=None, oracle=True):
    """breakSupport on chromosomes given as [(scaffold, row indices)] lists and [(scaffold, orientation)] arrangements,
    and the oracle on the same."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    binList, chromList, ordered = _explicit(host, groups, arrangements)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(host)
        results = p2.breakSupport(p2.GenomeMatrix(ctx), ordered, binList, chromList, minPiece=min_piece)
    where = {b.ID: i for i, b in enumerate(binList)}
    expected = [ref.oracle_breaks(host, where, rows, arr, min_piece, cuts)
                for rows, arr in zip(chromList, arrangements)] if oracle else None
    return results, expected


@pytest.fixture(scope="module")
def edges():
    """Scaffolds of 1, 2, 3 and 4 bins; a chromosome that is one scaffold (every candidate has a mirror image of the same
    objective); a chromosome of one bin; a chromosome without contacts; scaffolds long enough for minPiece = 3."""
    rng = np.random.default_rng(5)
    groups, arrs, pos = [], [], 0
    for prefix, lens in (("mix", [1, 2, 3, 4]), ("solo", [9]), ("bin", [1]), ("dark", [3, 2]), ("long", [7, 6, 2, 65])):
        g, pos = _chromosome(prefix, pos, lens)
        groups.append(g)
        order = rng.permutation(len(lens))
        arrs.append([(g[i][0], "-" if rng.random() < 0.5 else "+") for i in order])
    host = _decay_map(pos, 17)
    dark = [i for _name, idx in groups[3] for i in idx]
    host[np.ix_(dark, dark)] = 0.0                            # its total is 0: nothing to score
    return host, groups, arrs


def test_edge_shapes_in_one_call(edges):
    from hic_genome_assembler_amd import orderGenome as p2
    host, groups, arrs = edges
    results, expected = _run_explicit(host, groups, arrs)
    _compare(results, expected, "edges")
    by_bins = {r["bins"]: r for r in results[0]["rows"]}
    assert by_bins[1]["verdict"] == by_bins[2]["verdict"] == "NA" and by_bins[3]["best_cut"] is not None
    assert results[0]["table"].shape == (0 + 1 + 2 + 3, 8)
    solo = results[1]["rows"][0]
    print("one-scaffold chromosome: near count %d, best %s at cut %s" % (solo["near"], solo["best_move"], solo["best_cut"]))
    assert solo["near"] > 1 and solo["best_cut"] is not None  # mirror ties: decided on literal scores, as the oracle does
    assert results[2]["score0"] == 0.0 and results[2]["rows"][0]["verdict"] == "NA" and results[2]["table"].shape == (0, 8)
    assert results[3]["total"] == 0.0 and results[3]["score0"] == 0.0 and not results[3]["table"].any()
    assert [r["verdict"] for r in results[3]["rows"]] == ["NA", "NA"]
    text = p2.breakSupportText(results)
    assert _shape(text) == _shape(ref.report_text(expected))
    assert text.count("\tNA\tNA\tNA\tNA\tNA\tNA\n") == 2 + 1 + 2 + 1


def test_min_piece_keeps_the_table_and_narrows_the_best(edges):
    host, groups, arrs = edges
    one, _e = _run_explicit(host, groups, arrs, oracle=False)
    three, expected = _run_explicit(host, groups, arrs, min_piece=3)
    _compare(three, expected, "edges, minPiece 3")
    changed = 0
    for a, b in zip(one, three):
        assert np.array_equal(a["table"], b["table"]) and a["score0"] == b["score0"]
        for ra, rb in zip(a["rows"], b["rows"]):
            if rb["bins"] < 6:
                assert rb["verdict"] == "NA"
            elif rb["best_cut"] is not None:
                assert 3 <= rb["best_cut"] <= rb["bins"] - 3
                changed += ra["best_cut"] != rb["best_cut"]
    print("minPiece 3 against 1: best cuts that moved:", changed)
    assert [r["verdict"] != "NA" for r in three[4]["rows"]].count(True) == 3        # 7, 6 and 65 bins


@pytest.mark.parametrize("kind", ["decay", "ones"])
def test_best_is_the_summary_of_the_devices_own_table(kind):
    """The device's pick against its host restatement on the SAME doubles: ``best`` of hicmi_p2_breaks_multi equals
    break_summary of the blocks that call returned - integer equality, no tolerance, both sides evaluate
    top - |top| * NEAR_TOP on the same numbers.  8 (L - 1) candidates around the pick's 256-lane stride (L = 32, 33, 34),
    two strides (L = 65) and its exits (L = 2: nothing competes; L = 3), minPiece 1 and 3, one call each.  On the map of
    ones many scores are exactly equal: the first of equals wins and near counts above 1 must occur."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    groups, arrs, pos = [], [], 0
    for prefix, lens in (("a", [2, 33, 65]), ("b", [34, 3, 32])):
        g, pos = _chromosome(prefix, pos, lens)
        groups.append(g)
        arrs.append([(name, "-" if i == 1 else "+") for i, (name, _idx) in enumerate(g)])
    host = _decay_map(pos, 43) if kind == "decay" else np.ones((pos, pos))
    binList, chromList, ordered = _explicit(host, groups, arrs)
    near = 0
    with _lib.Context(0) as ctx:
        ctx.set_contacts(host)
        matrix = p2.GenomeMatrix(ctx)
        matrix.bin_index(binList)
        (jobs,) = p2._layout_jobs(matrix.lanes(len(ordered)), ordered, binList, chromList)
        lens = [[layout.length[int(i)] for i in ids] for layout, ids, _r, _t, _g in jobs]
        for min_piece in (1, 3):
            out = _lib.Context.p2_breaks_multi([(layout.ctx, ids, rev, ln, total) for (layout, ids, rev, total, _g), ln
                                                in zip(jobs, lens)], min_piece)
            for ln, (table, best) in zip(lens, out):
                off, n_rows = p2._break_offsets(ln)
                assert table.shape == (n_rows, 8) and np.isfinite(table).all()
                want = np.array([p2.break_summary(table[o:o + L - 1], L, min_piece) for o, L in zip(off, ln)], np.int32)
                assert np.array_equal(best, want), (min_piece, ln)
                near = max(near, int(best[:, 1].max()))
    print(kind, "map: largest near count", near)
    assert near > 1 or kind == "decay"


def _sample(j, L):
    return list(range(1, L)) if L <= 64 else sorted(set([1, 2, 3, L - 3, L - 2, L - 1] + list(range(37, L, 37))))


def test_a_scaffold_of_1100_bins_beside_a_chromosome_of_20(monkeypatch):
    """The mixed-size launch: one scaffold of 1,100 bins in a chromosome of 1,300 and a chromosome of 20
    bins in one hicmi_p2_breaks_multi call.  The oracle scores the first 3, the last 3 and every 37th cut of the scaffolds
    above 64 bins and every cut of the others; the best breaks are held to the DIRECT path."""
    big, pos = _chromosome("big", 0, [1100, 100, 60, 37, 1, 2])
    small, pos = _chromosome("small", pos, [7, 5, 1, 4, 3])
    arrs = [[("big2", "+"), ("big4", "+"), ("big0", "-"), ("big3", "-"), ("big5", "+"), ("big1", "+")],
            [("small2", "-"), ("small0", "+"), ("small4", "-"), ("small1", "+"), ("small3", "-")]]
    host = _decay_map(pos, 31)
    results, expected = _run_explicit(host, [big, small], arrs, cuts=_sample)
    assert expected[0]["n"] == 1300 and expected[1]["n"] == 20 and results[0]["rows"][2]["bins"] == 1100
    assert sum(e.get("sampled", False) for e in expected[0]["rows"].values()) == 2
    _compare(results, expected, "1,100-bin scaffold beside 20 bins, sampled")
    monkeypatch.setenv("HICMI_P2_BREAKS_DIRECT", "1")
    direct, _e = _run_explicit(host, [big, small], arrs, oracle=False)
    worst = 0.0
    for a, b in zip(results, direct):
        worst = max(worst, float(np.max(np.abs(a["table"] - b["table"]) / np.abs(b["table"]))))
        assert [(r["best_cut"], r["best_move"], r["verdict"]) for r in a["rows"]] == \
            [(r["best_cut"], r["best_move"], r["verdict"]) for r in b["rows"]]
        assert [r["best_delta"] for r in a["rows"]] == [r["best_delta"] for r in b["rows"]]
    print("1,100-bin scaffold: default against DIRECT, largest relative difference of a score %.3e; its best break: %s at %s"
          % (worst, results[0]["rows"][2]["best_move"], results[0]["rows"][2]["best_cut"]))
    assert worst <= REL


@pytest.mark.parametrize("name", ["n600", "n2000"])
def test_default_path_against_direct(name, tmp_path, monkeypatch):
    paths, groups, orders = _inputs(name, tmp_path)
    a = _breaks(paths, groups, orders, str(tmp_path / "a.txt"), fullDir=str(tmp_path / "full_a"))
    again = _breaks(paths, groups, orders, str(tmp_path / "a2.txt"), fullDir=str(tmp_path / "full_a2"))
    monkeypatch.setenv("HICMI_P2_BREAKS_DIRECT", "1")
    b = _breaks(paths, groups, orders, str(tmp_path / "b.txt"))
    worst = 0.0
    for x, y, z in zip(a, b, again):
        assert x["score0"] == y["score0"] and x["total"] == y["total"]
        assert np.array_equal(x["table"], z["table"])                       # a second call gives the same bits
        if y["score0"] != 0.0 and y["table"].size:
            worst = max(worst, float(np.max(np.abs(x["table"] - y["table"]) / np.abs(y["table"]))))
        for r, q in zip(x["rows"], y["rows"]):
            assert (r["best_cut"], r["best_move"], r["verdict"], r["bins"]) == (q["best_cut"], q["best_move"], q["verdict"], q["bins"])
    print(name, "default against DIRECT: largest relative difference of a score %.3e" % worst)
    assert worst <= REL
    texts = []
    for fn in ("a.txt", "b.txt", "a2.txt", os.path.join("full_a", "Chr_1.breaks.tsv"), os.path.join("full_a2", "Chr_1.breaks.tsv")):
        with open(str(tmp_path / fn)) as fh:
            texts.append(fh.read())
    assert texts[0] == texts[1] == texts[2]                   # the reported floats are literal scores on both paths
    assert texts[3] == texts[4] and len(texts[3].splitlines()) > 1


def test_part2_with_the_two_config_lines(tmp_path):
    """-part2 with breakSupportFile and brokenChromosomeGroupFile on n160: the golden outputs as before, and beside them
    the report and the broken group file that supportBreaks writes for that order; sweepPart2 -support writes the report too."""
    from hic_genome_assembler_amd import run_hicAssembler as run, supportBreaks as sb
    name = "n160"
    spec = gc.load_case(name)[0]
    paths, groups, orders = _inputs(name, tmp_path)
    cfg = _config(tmp_path, paths, groups, spec["n_scaffolds"], spec["scan_scaffolds"], breakSupportFile="breaks_part2.txt",
                  brokenChromosomeGroupFile="broken_part2.txt")
    out = str(tmp_path / "out")
    _quiet(run.main, ["-part2", "-config", cfg])
    v = run.readConfigFileToVariables(cfg)
    for key, fn in (("chromosomeOrderFile", "chromosomeOrders.txt"), ("plotOrderFile", "plotOrder.txt")):
        with open(v[key]) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn
    _quiet(sb.main, ["-config", cfg, "-chromosomeOrderFile", orders, "-out", os.path.join(out, "breaks_cli.txt"), "-broken",
                     os.path.join(out, "broken_cli.txt")])
    for a, b in (("breaks_part2.txt", "breaks_cli.txt"), ("broken_part2.txt", "broken_cli.txt")):
        with open(os.path.join(out, a)) as fa, open(os.path.join(out, b)) as fb:
            text = fa.read()
            assert text == fb.read() and text
    with open(os.path.join(out, "groups.txt")) as fh:
        assert fh.read() == gc.golden_text(name, "chromosomeGroups.txt")    # the group file itself is never changed
    # sweepPart2 -support at the one setting reproduces that order, and writes its report beside the placement support
    from hic_genome_assembler_amd import sweepPart2 as sw
    _quiet(sw.main, ["-config", cfg, "-out", os.path.join(out, "sweep"), "-support"])
    with open(os.path.join(out, "sweep", "best", "breakSupport.txt")) as fa, open(os.path.join(out, "breaks_cli.txt")) as fb:
        assert fa.read() == fb.read()
