"""The Part 1 parameter sweep (sweepPart1.py) on the CPU: grid parsing, deduplication, names, refusals, and full sweeps
through the oracle-backed fake context against oracle.run_part1 and the reference-written fixtures."""
import os

import pytest

import golden_cases as gc
import hic_oracle as orc
from fake_context import OracleContext

FILES = ("binGroups.txt", "assessment.txt", "chromosomeGroups.txt")


@pytest.fixture()
def fake_gpu(monkeypatch):
    from hic_genome_assembler_amd import _lib
    monkeypatch.setattr(_lib, "Context", OracleContext)
    monkeypatch.setattr(_lib, "hypergeom_sf", lambda x, M, n, N: float(orc.hyper_geom(x, M, n, N)))
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
    cfg = tmp_path / "cfg.txt"
    cfg.write_text("".join("%s = %s\n" % kv for kv in keys.items()))
    return str(cfg)


def test_parse_values_follows_the_config_rules(capsys):
    from hic_genome_assembler_amd import sweepPart1 as sw
    assert sw.parse_values("5,8, 10,8", "minSize", 5) == [5, 8, 10]
    assert sw.parse_values(".05,.01,0.05", "psig", .05) == [.05, .01]
    assert sw.parse_values("0,.05,0.0", "modularity", .05) == [0.0, .05]
    # modularity > 1 -> .05 with the parser's warning; psig > 1 keeps the config's value; a bad int keeps the config's
    assert sw.parse_values("2", "modularity", 0.0) == [.05]
    assert sw.parse_values("3,.01", "psig", .02) == [.02, .01]
    assert sw.parse_values("x,7", "minSize", 5) == [5, 7]
    assert "WARNING" in capsys.readouterr().out
    with pytest.raises(ValueError):
        sw.parse_values(" , ", "minSize", 5)


def test_grid_defaults_to_the_config_values(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run, sweepPart1 as sw
    paths = {k: "x" for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    v = run.readConfigFileToVariables(_config(tmp_path, paths, minSize="7", psig=".02", modularity=".1"))
    args = sw._parse_args(["-config", "c", "-psig", ".05,.01"])
    assert sw.grid_from_args(args, v) == ([7], [.05, .01], [.1], [20])
    args = sw._parse_args(["-config", "c", "-minSize", "3,5", "-louvainRounds", "4,8"])
    assert sw.grid_from_args(args, v) == ([3, 5], [.02], [.1], [4, 8])


def test_deduplication_of_the_scan_loops():
    from hic_genome_assembler_amd import sweepPart1 as sw
    n = 1000
    combos = sw.combinations([5, 8, 10, 15], [.05, .01, .001], [0.0, .05], [20])
    assert len(combos) == 24
    fp, keys = sw.plan(n, combos)
    assert len(fp) == 8                                     # (minSize, stop_ind): psig does not enter the first pass
    assert set(fp) == {(m, s) for m in (5, 8, 10, 15) for s in (1000, 950)}
    assert keys[0] == (5, 1000) and keys[1] == (5, 950)
    # modularity values that give the same stop_ind share a first pass; min_frac == 1 scans nothing
    fp, keys = sw.plan(n, sw.combinations([5], [.05], [.05, .0499, 1.0], [20]))
    assert len(fp) == 1 and keys == [(5, 950), (5, 950), None]


def test_directory_names():
    from hic_genome_assembler_amd import sweepPart1 as sw
    assert sw.combo_name(5, .05, 0.0) == "minSize5_psig0.05_modularity0"
    assert sw.combo_name(15, .001, .05) == "minSize15_psig0.001_modularity0.05"
    assert sw.combo_name(8, .01, .2, 20) == "minSize8_psig0.01_modularity0.2_louvainRounds20"


def test_refuses_hmm_and_shards(tmp_path, capsys):
    from hic_genome_assembler_amd import run_hicAssembler as run, sweepPart1 as sw
    paths = {k: "x" for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    v = run.readConfigFileToVariables(_config(tmp_path, paths, hyperGeom="False", hmm="True"))
    assert "hmm = True" in sw.check_config(v)
    v = run.readConfigFileToVariables(_config(tmp_path, paths, hyperGeom="False", hmm="False"))
    assert "hyperGeom = True" in sw.check_config(v)
    with pytest.raises(SystemExit):
        sw.main(["-config", _config(tmp_path, paths, hyperGeom="False", hmm="True")])
    assert "hmm = True is not supported" in capsys.readouterr().out
    with pytest.raises(ValueError, match="row shards"):
        sw.runSweep(*(["x"] * 8), [5], [.05], [0.0], [20], str(tmp_path), shard=(0, 2))


def _read(path):
    with open(path) as fh:
        return fh.read()


@pytest.mark.parametrize("name", ["n400_default", "n2000"])
def test_sweep_equals_the_oracle_per_combination(fake_gpu, name, tmp_path):
    from hic_genome_assembler_amd import sweepPart1 as sw
    spec, _meta, _gold, _lay, _c = gc.load_case(name)
    paths = gc.write_case_files(name, str(tmp_path))
    cfg = _config(tmp_path, paths, minSize=str(spec["min_size"]), psig=str(spec["psig"]))
    out = str(tmp_path / "sweep")
    minSizes = [3, 5, 8] if name == "n400_default" else [5, 8]
    sw.main(["-config", cfg, "-minSize", ",".join(map(str, minSizes)), "-psig", ".05,.01", "-modularity", "0",
             "-out", out])
    combos = sw.combinations(minSizes, [.05, .01], [0.0], [20])
    rows = sw.read_summary(os.path.join(out, "sweep_summary.tsv"))
    assert len(rows) == len(combos)
    assert _read(str(tmp_path / "files" / "dendrogramOrder.txt")) == gc.golden_text(name, "dendrogramOrder.txt")
    matched_fixture = False
    for (ms, ps, mod, _lr), row in zip(combos, rows):
        d = os.path.join(out, sw.combo_name(ms, ps, mod))
        ref = tmp_path / ("oracle_%d_%g" % (ms, ps))
        ref.mkdir()
        r = lambda fn: str(ref / fn)  # noqa: E731
        cuts = orc.run_part1(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                             paths["hicProScaffSizeFile"], r("dendrogramOrder.txt"), r("binGroups.txt"),
                             r("assessment.txt"), r("chromosomeGroups.txt"), min_size=ms, modularity=0.0, psig=ps)
        for fn in FILES:
            assert _read(os.path.join(d, fn)) == _read(r(fn)), (ms, ps, fn)
        if ms == spec["min_size"] and ps == spec["psig"]:
            matched_fixture = True
            for fn in FILES:
                assert _read(os.path.join(d, fn)) == gc.golden_text(name, fn), fn
        # the summary row matches the files
        assert (int(row["minSize"]), float(row["psig"]), float(row["modularity"])) == (ms, ps, mod)
        assert row["cut_indices"] == [int(v) for v in cuts]
        assert int(row["filtered_cuts"]) == len(cuts) and int(row["louvain_groups"]) == 0
        bg = _read(os.path.join(d, "binGroups.txt"))
        assert int(row["groups"]) == bg.count("### Chromosome group ")
        assessment = _read(os.path.join(d, "assessment.txt"))
        assert assessment.splitlines()[-2] == "Total scaffolds assigned to chromosomes " + row["scaffolds_assigned"]
        groups, cur = [], set()
        for line in bg.splitlines()[1:]:
            if line.startswith("#"):
                groups.append(cur)
                cur = set()
            else:
                cur.add(line.split("\t")[1])
        groups.append(cur)
        split = {s for s in set().union(*groups) if sum(s in g for g in groups) > 1}
        assert int(row["split_scaffolds"]) == len(split)
        log = _read(os.path.join(d, "part1.log")).splitlines()
        assert log[-1] == "%d chromosomes read in from file" % len(groups)
        assert "- Filtered cut indices {}".format([int(v) for v in cuts]) in log
        assert sum(ln.startswith("- Breakpoints found") for ln in log) == 1
        assert int(row["first_pass_cuts"]) == int([ln for ln in log if ln.startswith("- Breakpoints found")][0].split()[-1])
    assert matched_fixture


def test_sweep_log_equals_a_standalone_run(fake_gpu, tmp_path, capsys):
    """part1.log holds the scan and assessment lines a -part1 run with that config prints (run-time lines left out)."""
    from hic_genome_assembler_amd import run_hicAssembler as run, sweepPart1 as sw
    name = "n400_default"
    paths = gc.write_case_files(name, str(tmp_path))
    out = str(tmp_path / "sweep")
    sw.main(["-config", _config(tmp_path, paths), "-minSize", "3,5", "-psig", ".01", "-out", out])
    for ms in (3, 5):
        capsys.readouterr()
        run.main(["-part1", "-config", _config(tmp_path, paths, minSize=str(ms), psig=".01")])
        printed = capsys.readouterr().out.splitlines()
        want = [ln for ln in printed if ln.startswith("- ") and not sw._is_runtime_line(ln)
                and not ln.startswith("- Part 1")] + [ln for ln in printed if ln.endswith("chromosomes read in from file")]
        d = os.path.join(out, sw.combo_name(ms, .01, 0.0))
        assert _read(os.path.join(d, "part1.log")).splitlines() == want
        for fn in FILES:
            assert _read(os.path.join(d, fn)) == _read(str(tmp_path / "files" / fn)), fn
