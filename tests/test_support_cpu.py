"""Placement support (orderGenome.placementSupport, supportPart2.py) on the CPU: the host logic above hicmi_p2_support -
enumeration order, which candidates compete for a scaffold's best move, verdicts, the report text, the command line and
the config key - through a fake context that answers p2_support with the oracle, held to tests/support_reference.py."""
import os

import numpy as np
import pytest

import golden_cases as gc
import support_reference as ref
from fake_context import OracleContext

NEAR_TOP = 1e-9


class SupportContext(OracleContext):
    """OracleContext that also answers p2_support: every candidate's bin order built explicitly and scored literally;
    `best` restated here from the bin orders themselves."""

    def p2_support(self, ids, rev, total):
        ids, rev = [int(v) for v in ids], [int(v) for v in rev]
        self.p2_set_arrangement(ids, rev)
        S = len(ids)
        pieces = [(self._positions(i, 0), bool(r)) for i, r in zip(ids, rev)]
        row0 = self._row(ids, rev)
        table, best = np.zeros((S, S, 2)), np.tile(np.array([-1, 0], np.int32), (S, 1))
        if len(row0) < 2 or not total > 0:
            return table, best
        for j in range(S):
            cand = [ref.candidate_row(pieces, j, g, r) for g in range(S) for r in (0, 1)]
            vals = self._literal(np.stack(cand), total)
            table[j] = vals.reshape(S, 2)
            seen, counted = {row0.tobytes()}, []
            for i, c in enumerate(cand):                     # a bin order counts once, where it is enumerated first
                if S > 1 and c.tobytes() not in seen:
                    seen.add(c.tobytes())
                    counted.append(i)
            if counted:
                v = vals[counted]
                top = float(v.max())
                best[j] = (counted[int(np.argmax(v))], int(np.count_nonzero(v >= top - abs(top) * NEAR_TOP)))
        return table, best


@pytest.fixture()
def fake_gpu(monkeypatch):
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    monkeypatch.setattr(_lib, "Context", SupportContext)
    monkeypatch.setattr(p2, "WORKERS", 1)
    monkeypatch.delenv("HICMI_P2_SUPPORT_DIRECT", raising=False)
    return _lib


def _config(tmp_path, paths, **over):
    keys = dict(resolution="100000", saveFilesDirectory=str(tmp_path / "files"), savePlotsDirectory=str(tmp_path / "plots"),
                hicProBedFile=paths["hicProBedFile"], hicProBiasFile=paths["hicProBiasFile"],
                hicProMatrixFile=paths["hicProMatrixFile"], hicProScaffSizeFile=paths["hicProScaffSizeFile"],
                dendrogramOrderFile="dendrogramOrder.txt", avgClusterPlot="a.png", avgClusterPlot_outlined="b.png",
                binGroupFile="binGroups.txt", assessmentFile="assessment.txt", hyperGeom="True", hmm="False",
                minSize="5", modularity="0", psig=".05", convergenceRounds="5", lookAhead=".2", louvainRounds="20",
                chromosomeGroupFile="chromosomeGroups.txt", chromosomeOrderFile="chromosomeOrders.txt",
                chromosomePlotSuffix="synthetic", fullGenomePlot="g.png", fullGenomePlotTitle="t",
                plotOrderFile="plotOrder.txt", nScaffolds="6", scanScaffolds="5", lengthCutoff="500000",
                restrictionSiteFile="x", validPairFile="x", finalOrderingsFile="final.txt", originalFastaFile="x",
                assembledFastaFile="out.fa")
    keys.update(over)
    os.makedirs(keys["saveFilesDirectory"], exist_ok=True)
    os.makedirs(keys["savePlotsDirectory"], exist_ok=True)
    cfg = tmp_path / "cfg.txt"
    cfg.write_text("".join("%s = %s\n" % kv for kv in keys.items()))
    return str(cfg), keys["saveFilesDirectory"]


def _golden_inputs(name, tmp_path):
    """The case's HiC-Pro files, its golden group and order files in saveFilesDirectory, and the config."""
    paths = gc.write_case_files(name, str(tmp_path))
    cfg, files = _config(tmp_path, paths)
    for fn in ("chromosomeGroups.txt", "chromosomeOrders.txt"):
        with open(os.path.join(files, fn), "w") as fh:
            fh.write(gc.golden_text(name, fn))
    return paths, cfg, files


_reference = ref.reference_for_files


def _assert_same(results, expected):
    assert len(results) == len(expected)
    for got, exp in zip(results, expected):
        assert got["names"] == exp["names"] and got["orientations"] == exp["orientations"]
        assert got["total"] == exp["total"] and got["score0"] == exp["score0"]
        assert np.array_equal(got["table"], exp["table"])           # both sides are the oracle's literal values
        for j, row in enumerate(got["rows"]):
            e = exp["rows"][j]
            assert row["bins"] == e["bins"] and row["flip_delta"] == e["flip_delta"] and row["verdict"] == e["verdict"]
            if e["best"] is None:
                assert row["best_gap"] is None and row["best_orientation"] is None and row["best_delta"] is None
            else:
                assert (row["best_gap"], row["best_orientation"], row["best_delta"]) == e["best"]


def test_report_of_the_n160_golden_order(fake_gpu, tmp_path):
    from hic_genome_assembler_amd import supportPart2 as sp
    paths, cfg, files = _golden_inputs("n160", tmp_path)
    out = os.path.join(files, "support.txt")
    sp.main(["-config", cfg, "-out", out, "-full", os.path.join(files, "full")])
    expected = _reference(paths, os.path.join(files, "chromosomeGroups.txt"), os.path.join(files, "chromosomeOrders.txt"))
    with open(out) as fh:
        text = fh.read()
    assert text == ref.report_text(expected)
    lines = text.splitlines()
    assert sum(1 for ln in lines if ln.startswith("### Chromosome grouping ")) == len(expected)
    assert all(len(ln.split("\t")) == 8 for ln in lines if not ln.startswith("#"))
    one_bin = [ln for ln in lines if not ln.startswith("#") and ln.split("\t")[2] == "1"]
    assert one_bin and all(ln.split("\t")[3] == "0.0" and ln.split("\t")[7] in ("orientation_open", "improvable") for ln in one_bin)
    # -full: one S x 2S table per chromosome, rows in arrangement order, gap ascending, '+' before '-'
    for k, exp in enumerate(expected):
        with open(os.path.join(files, "full", "Chr_%d.support.tsv" % (k + 1))) as fh:
            rows = [ln.rstrip("\n").split("\t") for ln in fh]
        S = len(exp["names"])
        assert rows[0] == ["scaffold"] + ["gap%d%s" % (g, o) for g in range(S) for o in "+-"]
        assert [r[0] for r in rows[1:]] == exp["names"]
        assert np.array_equal(np.array([[float(v) for v in r[1:]] for r in rows[1:]]), exp["table"].reshape(S, 2 * S))


def test_host_logic_matches_the_reference_on_a_perturbed_order(fake_gpu, tmp_path):
    """Swapping two multi-bin scaffolds and flipping a third gives improvable rows: positive deltas, moves and verdicts."""
    from hic_genome_assembler_amd import supportPart2 as sp
    paths, cfg, files = _golden_inputs("n160", tmp_path)
    groups = ref.read_group_file(os.path.join(files, "chromosomeGroups.txt"))
    orders = ref.read_order_file(os.path.join(files, "chromosomeOrders.txt"))
    c, _a, _b, f = ref.perturb(groups, orders)
    pert = os.path.join(files, "perturbed.txt")
    ref.write_order_file(pert, orders)
    results = sp.runSupport(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                            os.path.join(files, "chromosomeGroups.txt"), pert, os.path.join(files, "s.txt"))
    expected = _reference(paths, os.path.join(files, "chromosomeGroups.txt"), pert)
    _assert_same(results, expected)
    verdicts = [r["verdict"] for r in results[c]["rows"]]
    assert verdicts.count("improvable") >= 2
    assert results[c]["rows"][f]["flip_delta"] > 0


def _bins(n):
    from hic_genome_assembler_amd.hostio import Bin
    return [Bin(100 + i, "c", i, i + 1, 1.0, 0.0) for i in range(n)]


def _small_map(n, seed):
    rng = np.random.default_rng(seed)
    d = np.abs(np.subtract.outer(np.arange(n), np.arange(n)))
    c = rng.uniform(0.5, 1.5, (n, n)) * 100.0 / (1.0 + d) ** 1.2
    return np.ascontiguousarray(0.5 * (c + c.T))


def _run(host, groups, arrangements):
    """placementSupport on explicit chromosomes: groups = [[(scaffold, bins as row indices)]] in group-file order,
    arrangements = [[(scaffold, orientation)]]."""
    from hic_genome_assembler_amd import orderGenome as p2
    binList = _bins(len(host))
    ctx = SupportContext()
    ctx.set_contacts(host)
    chromList = [[[binList[i].ID, name] for name, idx in g for i in idx] for g in groups]
    chromList = [sorted(rows) for rows in chromList]
    ordered = []
    for rows, arr in zip(chromList, arrangements):
        scaffs = []
        for name, o in arr:
            s = p2.Scaffold(name, sorted(b for b, x in rows if x == name), "+")
            if o == "-":
                s.flipOrientation()
            scaffs.append(s)
        ordered.append(scaffs)
    results = p2.placementSupport(p2.GenomeMatrix(ctx), ordered, binList, chromList)
    where = {b.ID: i for i, b in enumerate(binList)}
    expected = [ref.oracle_support(host, where, rows, arr) for rows, arr in zip(chromList, arrangements)]
    return results, expected


def test_one_and_two_scaffold_chromosomes_and_one_bin_scaffolds(fake_gpu):
    host = _small_map(23, 5)
    groups = [[("solo", range(0, 6))],                                     # S = 1: nothing to compare with
              [("a", range(6, 10)), ("b", range(10, 13))],                 # S = 2
              [("p", [13]), ("q", [14]), ("r", [15]), ("s", [16])],        # one-bin scaffolds only
              [("lone", [17])],                                            # fewer than 2 bins: total 0.0, no candidates
              [("x", range(18, 21)), ("y", [21]), ("z", [22])]]
    arrs = [[("solo", "-")], [("b", "-"), ("a", "+")], [("q", "+"), ("p", "-"), ("s", "+"), ("r", "-")], [("lone", "+")],
            [("y", "-"), ("x", "-"), ("z", "+")]]
    results, expected = _run(host, groups, arrs)
    _assert_same(results, expected)
    solo = results[0]["rows"][0]
    assert solo["best_gap"] is None and solo["verdict"] == "orientation_open" and solo["flip_delta"] == 0.0
    assert results[0]["table"].shape == (1, 1, 2)
    assert results[0]["table"][0, 0, 1] == results[0]["score0"]            # (g = j, own orientation) is the arrangement
    two = results[1]
    assert two["table"].shape == (2, 2, 2) and all(r["best_gap"] is not None for r in two["rows"])
    for row in results[2]["rows"]:                                         # every in-place flip ties: exactly 0.0
        assert row["flip_delta"] == 0.0 and row["verdict"] in ("orientation_open", "improvable")
        assert row["best_orientation"] == "+"                              # '-' is the same bin order and comes second
    assert results[3]["score0"] == 0.0 and results[3]["total"] == 0.0
    assert results[3]["rows"][0]["best_gap"] is None and results[3]["rows"][0]["verdict"] == "orientation_open"
    from hic_genome_assembler_amd import orderGenome as p2
    text = p2.placementSupportText(results)
    assert text == ref.report_text(expected)
    assert "solo\t-\t6\t" in text and "\tNA\tNA\tNA\t" in text


def test_enumeration_order_and_exclusions():
    from hic_genome_assembler_amd import orderGenome as p2
    lengths, rev = [3, 1, 2], [1, 0, 0]
    m = p2.support_counts(lengths, rev)
    assert m.shape == (3, 3, 2)
    assert not m[0, 0, 1] and m[0, 0, 0]                    # own gap, own orientation is the arrangement; the flip counts
    assert not m[1, 1].any() and not m[1, :, 1].any() and m[1, 0, 0] and m[1, 2, 0]     # one bin: '+' elsewhere only
    assert not m[2, 2, 0] and m[2, 2, 1]
    table = np.zeros((3, 3, 2))
    table[0, 0, 1] = 9.0                                    # the arrangement itself never wins
    table[0, 1, 0] = table[0, 1, 1] = 5.0                   # a tie: the first in enumeration order, both within the band
    table[1, 2, 1] = 7.0                                    # a one-bin scaffold's '-' does not count
    table[1, 2, 0] = 6.0
    table[2, 0, 1] = 4.0
    table[2, 0, 0] = 4.0 * (1 - 5e-10)
    best = p2.support_summary(table, lengths, rev)
    assert best.tolist() == [[2, 2], [4, 1], [1, 2]]


def test_near_ties_are_decided_on_literal_scores(fake_gpu):
    """A best move with rivals within 1e-9 is re-scored with p2_score_exact: the first strict maximum of those wins."""
    from hic_genome_assembler_amd import orderGenome as p2
    host = _small_map(9, 3)
    binList = _bins(9)
    ctx = SupportContext()
    ctx.set_contacts(host)
    scaffs = [p2.Scaffold("a", [100, 101, 102], "+"), p2.Scaffold("b", [103, 104], "+"), p2.Scaffold("c", [105, 106, 107, 108], "+")]
    chromList = [[[b, s.name] for s in scaffs for b in s.binList]]
    calls = []
    honest = SupportContext.p2_support

    def tilted(self, ids, rev, total):
        table, best = honest(self, ids, rev, total)
        # a closed form that ranks scaffold 0's true runner-up first by less than the band
        order = np.argsort(-np.where(p2.support_counts([3, 2, 4], rev)[0].reshape(-1), table[0].reshape(-1), -np.inf))
        first, second = int(order[0]), int(order[1])
        table = table.copy()
        table[0].reshape(-1)[second] = table[0].reshape(-1)[first] * (1 + 1e-12)
        best = best.copy()
        best[0] = (second, 2)
        calls.append((first, second))
        return table, best
    SupportContext.p2_support = tilted
    try:
        res = p2.placementSupport(p2.GenomeMatrix(ctx), [scaffs], binList, chromList)[0]
    finally:
        SupportContext.p2_support = honest
    first, _second = calls[0]
    assert (res["rows"][0]["best_gap"], res["rows"][0]["best_orientation"]) == (first // 2, "-" if first % 2 else "+")


def test_order_file_reader_checks_the_group_file(tmp_path):
    from hic_genome_assembler_amd import orderGenome as p2
    chromList = [[[1, "a"], [2, "a"], [3, "b"]], [[4, "c"]]]
    good = tmp_path / "o.txt"
    good.write_text("### Chromosome grouping 1 ###\nb\t-\na\t-\n### Chromosome grouping 2 ###\nc\t+\n")
    out = p2.scaffoldsFromOrderFile(chromList, str(good))
    assert [[(s.name, s.orientation, s.binList) for s in g] for g in out] == [[("b", "-", [3]), ("a", "-", [2, 1])], [("c", "+", [4])]]
    bad = tmp_path / "bad.txt"
    bad.write_text("### Chromosome grouping 1 ###\nb\t-\n### Chromosome grouping 2 ###\nc\t+\n")
    with pytest.raises(ValueError):
        p2.scaffoldsFromOrderFile(chromList, str(bad))
    bad.write_text("### Chromosome grouping 1 ###\nb\t-\na\t-\n")
    with pytest.raises(ValueError):
        p2.scaffoldsFromOrderFile(chromList, str(bad))


def test_command_line_and_config_handling(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run, supportPart2 as sp
    paths = gc.write_case_files("n160", str(tmp_path))
    cfg, files = _config(tmp_path, paths)
    v = run.readConfigFileToVariables(cfg)
    assert "placementSupportFile" not in v and not run.ensureAllVariablesAreSet(v)
    args = sp._parse_args(["-config", cfg])
    assert (args.device, args.full, args.out, args.chromosomeOrderFile) == (0, None, None, None)
    assert sp.resolve(args, v) == (files + "/chromosomeOrders.txt", os.path.join(files, "placementSupport.txt"))
    args = sp._parse_args(["-config", cfg, "-chromosomeOrderFile", "ref.txt", "-out", "o.txt", "-full", "d", "-device", "2"])
    assert sp.resolve(args, v) == ("ref.txt", "o.txt") and args.full == "d" and args.device == 2
    cfg2, files = _config(tmp_path, paths, placementSupportFile="support.txt")
    v2 = run.readConfigFileToVariables(cfg2)
    assert v2["placementSupportFile"] == files + "/support.txt" and not run.ensureAllVariablesAreSet(v2)
    assert sp.resolve(sp._parse_args(["-config", cfg2]), v2)[1] == files + "/support.txt"
    assert {k: x for k, x in v2.items() if k != "placementSupportFile"} == v
    with pytest.raises(SystemExit):
        sp._parse_args([])


def test_part2_without_the_key_writes_the_golden_files_and_no_report(fake_gpu, tmp_path, capsys):
    from hic_genome_assembler_amd import run_hicAssembler as run
    paths, cfg, files = _golden_inputs("n160", tmp_path)
    os.remove(os.path.join(files, "chromosomeOrders.txt"))
    run.main(["-part2", "-config", cfg])
    plain = capsys.readouterr().out
    assert sorted(os.listdir(files)) == ["chromosomeGroups.txt", "chromosomeOrders.txt", "plotOrder.txt"]
    for fn in ("chromosomeOrders.txt", "plotOrder.txt"):
        with open(os.path.join(files, fn)) as fh:
            assert fh.read() == gc.golden_text("n160", fn), fn
    assert "Placement support" not in plain
    # with the key: the same two files, the report beside them, and it is supportPart2's
    cfg2, _ = _config(tmp_path, paths, placementSupportFile="support.txt")
    run.main(["-part2", "-config", cfg2])
    assert "Placement support written for scaffolds" in capsys.readouterr().out
    for fn in ("chromosomeOrders.txt", "plotOrder.txt"):
        with open(os.path.join(files, fn)) as fh:
            assert fh.read() == gc.golden_text("n160", fn), fn
    expected = _reference(paths, os.path.join(files, "chromosomeGroups.txt"), os.path.join(files, "chromosomeOrders.txt"))
    with open(os.path.join(files, "support.txt")) as fh:
        assert fh.read() == ref.report_text(expected)
