"""The Part 2 parameter sweep (sweepPart2.py) on the CPU: grid parsing, the clamps and folding, names, refusals, the
sharing planner, the summary and the best-pick rule, and full sweeps through the oracle-backed fake context against
oracle.run_part2, the reference-written fixtures and one-worker standalone runs."""
import contextlib
import io
import os

import pytest

import golden_cases as gc
import hic_oracle as orc
from fake_context import OracleContext

FILES = ("chromosomeOrders.txt", "plotOrder.txt")


@pytest.fixture()
def fake_gpu(monkeypatch):
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    monkeypatch.setattr(_lib, "Context", OracleContext)
    monkeypatch.setattr(p2, "WORKERS", 1)
    return _lib


def _config(tmp_path, paths, groups, **over):
    keys = dict(resolution="100000", saveFilesDirectory=str(tmp_path / "files"), savePlotsDirectory=str(tmp_path / "plots"),
                hicProBedFile=paths["hicProBedFile"], hicProBiasFile=paths["hicProBiasFile"],
                hicProMatrixFile=paths["hicProMatrixFile"], hicProScaffSizeFile=paths["hicProScaffSizeFile"],
                dendrogramOrderFile="dendrogramOrder.txt", avgClusterPlot="a.png", avgClusterPlot_outlined="b.png",
                binGroupFile="binGroups.txt", assessmentFile="assessment.txt", hyperGeom="True", hmm="False",
                minSize="5", modularity="0", psig=".05", convergenceRounds="5", lookAhead=".2", louvainRounds="20",
                chromosomeGroupFile=groups, chromosomeOrderFile="chromosomeOrders.txt",
                chromosomePlotSuffix="synthetic", fullGenomePlot="g.png", fullGenomePlotTitle="t",
                plotOrderFile="plotOrder.txt", nScaffolds="6", scanScaffolds="5", lengthCutoff="500000",
                restrictionSiteFile="x", validPairFile="x", finalOrderingsFile="final.txt", originalFastaFile="x",
                assembledFastaFile="out.fa")
    keys.update(over)
    os.makedirs(keys["saveFilesDirectory"], exist_ok=True)
    cfg = tmp_path / "cfg.txt"
    cfg.write_text("".join("%s = %s\n" % kv for kv in keys.items()))
    return str(cfg)


def test_grid_clamps_and_folding():
    from hic_genome_assembler_amd import sweepPart2 as sw
    grid, folded = sw.settings([5, 6, 9, 8], [4, 8, 9])
    assert grid == [(5, 4), (5, 5), (6, 4), (6, 6), (8, 4), (8, 8)]
    assert folded[(5, 5)] == [(5, 8), (5, 9)]
    assert folded[(8, 8)] == [(9, 8), (9, 9), (8, 8), (8, 9)]
    assert (5, 4) not in folded
    assert sw.clamp(12, 3) == (8, 3) and sw.clamp(4, 7) == (4, 4)
    assert sw.setting_name(8, 7) == "nScaffolds8_scanScaffolds7"


def test_grid_defaults_to_the_config_values(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run, sweepPart2 as sw
    paths = {k: "x" for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    v = run.readConfigFileToVariables(_config(tmp_path, paths, "g.txt", nScaffolds="7", scanScaffolds="4"))
    assert sw.grid_from_args(sw._parse_args(["-config", "c"]), v) == ([7], [4])
    args = sw._parse_args(["-config", "c", "-scanScaffolds", "3,5,3", "-chromosomeGroupFile", "other.txt"])
    assert sw.grid_from_args(args, v) == ([7], [3, 5])
    assert args.chromosomeGroupFile == "other.txt"


def test_refuses_row_shards(tmp_path):
    from hic_genome_assembler_amd import sweepPart2 as sw
    with pytest.raises(ValueError, match="one GPU"):
        sw.runSweep("b", "c", "m", "g", "o", "p", [6], [5], str(tmp_path), shard=(0, 2))


def test_planner_shares_brute_force_insertion_and_scans():
    from hic_genome_assembler_amd import sweepPart2 as sw
    grid, _ = sw.settings([3, 4, 6], [2, 3, 5])
    counts = [2, 4, 5, 9]                  # S < every nS; S = 4; S = 5 (between); S > every nS
    starts, scans, per_setting = sw.plan(counts, grid)
    # chromosome 0 (2 scaffolds): one brute force of width 2 serves every setting, never scanned
    assert [k for k in starts if k[0] == 0] == [(0, 2)]
    assert [k for k in scans if k[0] == 0] == [(0, 2, None)]
    # chromosome 1 (4 scaffolds): widths 3 and 4; scans only at nS = 3
    assert [k for k in starts if k[0] == 1] == [(1, 3), (1, 4)]
    assert sorted(k for k in scans if k[0] == 1) == [(1, 3, 2), (1, 3, 3), (1, 4, None)]
    # chromosome 3 (9 scaffolds): every setting scans; widths 3, 4, 6
    assert [k for k in starts if k[0] == 3] == [(3, 3), (3, 4), (3, 6)]
    assert len([k for k in scans if k[0] == 3]) == len(grid)
    assert len(starts) < len(grid) * len(counts) and len(scans) < len(grid) * len(counts)
    assert all(len(keys) == len(counts) for keys in per_setting)
    assert all(scans[fk] == sw.start_key(fk[0], counts[fk[0]], g[0]) for g, keys in zip(grid, per_setting) for fk in keys)


def test_best_pick_prefers_the_earlier_setting_on_a_tie(tmp_path):
    from hic_genome_assembler_amd import sweepPart2 as sw
    scores = [[1.0, 2.0, 3.0], [1.0, 2.5, 2.0], [0.5, 2.5, 3.0]]
    assert sw.best_settings(scores) == [0, 1, 0]
    grid = [(4, 3), (6, 5), (8, 8)]
    res = {"scores": scores, "scanned": [[True, False, True]] * 3, "rounds": [[2, 0, 1]] * 3}
    chroms = [[(1, "a"), (2, "b")], [(3, "c")], [(4, "d"), (5, "d")]]
    sw.write_summary(str(tmp_path), grid, res, chroms, sw.best_settings(scores))
    rows = sw.read_summary(str(tmp_path / "sweep_summary.tsv"))
    assert [(r["nScaffolds"], r["scanScaffolds"], r["best_for"]) for r in rows] == [("4", "3", "2"), ("6", "5", "1"),
                                                                                  ("8", "8", "0")]
    assert [r["final_scores"] for r in rows] == scores
    assert rows[0]["chromosomes_scanned"] == "2" and rows[0]["scan_rounds"] == "3"
    lines = (tmp_path / "chromosome_scores.tsv").read_text().splitlines()
    assert lines[2].split("\t") == ["2", "1", "1", "2.0", "2.5", "2.5", "nScaffolds6_scanScaffolds5"]


def part2_log(text):
    """The lines of a one-worker -part2 run from "Chromosomes found" to the last "Final ordering" block."""
    lines = text.splitlines()
    a = next(i for i, ln in enumerate(lines) if ln.startswith("Chromosomes found"))
    b = next(i for i, ln in enumerate(lines) if ln.startswith("RunTime for total genome"))
    return lines[a:b]


@pytest.mark.parametrize("case", ["n160", "n400_default"])
def test_sweep_matches_oracle_and_standalone_runs(case, tmp_path, fake_gpu):
    from hic_genome_assembler_amd import orderGenome as p2, sweepPart2 as sw
    spec = gc.load_case(case)[0]
    paths = gc.write_case_files(case, str(tmp_path))
    groups = tmp_path / "chromosomeGroups.txt"
    groups.write_text(gc.golden_text(case, "chromosomeGroups.txt"))
    out = tmp_path / "sweep"
    nS, sc = [3, 4, 6], [2, 3, 5]
    if (spec["n_scaffolds"], spec["scan_scaffolds"]) not in sw.settings(nS, sc)[0]:
        nS, sc = nS + [spec["n_scaffolds"]], sc + [spec["scan_scaffolds"]]
    with contextlib.redirect_stdout(io.StringIO()):
        res = sw.runSweep(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], str(groups),
                          "chromosomeOrders.txt", "plotOrder.txt", nS, sc, str(out))
    grid = res["grid"]
    assert res["counts"]["start_jobs"] < len(grid) * len(res["orders"][0])
    for g in grid:
        d = out / sw.setting_name(*g)
        ref = tmp_path / ("oracle_%d_%d" % g)
        ref.mkdir()
        orc.run_part2(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], str(groups),
                      str(ref / FILES[0]), str(ref / FILES[1]), n_scaffolds=g[0], scan_scaffolds=g[1], batch=True)
        for f in FILES:
            assert (d / f).read_text() == (ref / f).read_text(), (g, f)
        if g == (spec["n_scaffolds"], spec["scan_scaffolds"]):
            for f in FILES:
                assert (d / f).read_text() == gc.golden_text(case, f), (g, f)
        # part2.log = a one-worker standalone run's lines
        solo = tmp_path / ("solo_%d_%d" % g)
        solo.mkdir()
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            p2.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], str(groups),
                           str(solo / FILES[0]), False, False, False, "t", str(solo / FILES[1]), g[0], g[1], 100000)
        assert (d / "part2.log").read_text().splitlines() == part2_log(buf.getvalue()), g
        for f in FILES:
            assert (d / f).read_text() == (solo / f).read_text(), (g, f)
    # best/: each chromosome's pieces from its highest-scoring setting
    best = res["best"]
    rows = sw.read_summary(str(out / "sweep_summary.tsv"))
    assert len(rows) == len(grid)
    for c in range(len(best)):
        scores = [r["final_scores"][c] for r in rows]
        assert best[c] == scores.index(max(scores))
    chunks = (out / "best" / FILES[0]).read_text().split("### Chromosome grouping ")[1:]
    for c, chunk in enumerate(chunks):
        want = (out / sw.setting_name(*grid[best[c]]) / FILES[0]).read_text().split("### Chromosome grouping ")[c + 1]
        assert chunk == want, c
