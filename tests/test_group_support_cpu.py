"""Group support (scaffoldToChromosomes.groupSupport, supportPart1.py) on the CPU: the host logic above
hicmi_group_sums - labels, counts, densities, verdicts, the two files, the command line and the config keys - through a
NumPy double of ``group_sums`` kept in this file, held to tests/group_support_reference.py.

Verdict counts of the golden group files: the figures of the definition's prototype, except n300_edges.  For that case
the prototype's figures (35 supported, 3 contested, 4 ambiguous, 1 rescued) presume five scaffolds outside every group;
the committed tests/golden/n300_edges/chromosomeGroups.txt names all 43 scaffolds (its assessment.txt ends with "Total
scaffolds assigned to chromosomes 43"), so none can be ambiguous or rescued.  Its three zero rows do not move the counts
(L_s = all bins of a scaffold or only its non-zero rows: the same verdicts, checked below); the counts recorded here
are those of the reference module: 40 supported, 3 contested.
Leave-out figures (withheld, rescued, wrong) of the reference module: n300_edges (9, 5, 0), n400_default (10, 8, 0),
n600 (12, 7, 0), n2000 (34, 27, 0), n500_sparse (14, 13, 0): inside the two conditions asserted below."""
import os

import numpy as np
import pytest

import golden_cases as gc
import group_support_reference as ref

COUNTS = {"n160": dict(supported=30),
          "n300_edges": dict(supported=40, contested=3),
          "n400_default": dict(supported=46, contested=3, ambiguous=1),
          "n500_sparse": dict(supported=66, contested=1),
          "n600": dict(supported=52, contested=5),
          "n2000": dict(supported=161, contested=6)}
LEAVE_OUT = ["n300_edges", "n400_default", "n600", "n2000", "n500_sparse"]


class NumpyContext:
    """What groupSupport and the drivers need of _lib.Context, in NumPy: the sums in the definition's order, written as
    plain loops over chunks and rows."""

    def __init__(self, device=0):
        self.n, self.M = 0, None

    def set_contacts(self, mat):
        self.M = np.array(mat, dtype=np.float64)
        self.n = len(self.M)

    def row_sums(self):
        s = self.M.sum(axis=1)
        return s, s.copy()

    def compact(self, keep):
        self.M = np.ascontiguousarray(self.M[np.ix_(keep, keep)])
        self.n = len(self.M)

    def group_sums(self, grp, scaf, n_groups, n_scaffolds, want_bins=True):
        grp, scaf = np.asarray(grp), np.asarray(scaf)
        assert grp.shape == scaf.shape == (self.n,)
        assert grp.min() >= -1 and grp.max() < n_groups and scaf.min() >= 0 and scaf.max() < n_scaffolds
        binsum = np.zeros((self.n, n_groups))
        for g in range(n_groups):
            rows = np.flatnonzero(grp == g)
            total = np.zeros(self.n)
            for c0 in range(0, len(rows), 64):
                acc = np.zeros(self.n)
                for j in rows[c0:c0 + 64]:
                    acc = acc + np.where(scaf != scaf[j], self.M[j], 0.0)
                total = total + acc
            binsum[:, g] = total
        scafsum = np.zeros((n_scaffolds, n_groups))
        for i in range(self.n):
            scafsum[scaf[i]] = scafsum[scaf[i]] + binsum[i]
        return (binsum if want_bins else None), scafsum

    def close(self):
        pass


class _Matrix:
    def __init__(self, M):
        self.ctx = NumpyContext()
        self.ctx.set_contacts(M)
        self.np_sum = None


@pytest.fixture()
def fake_gpu(monkeypatch):
    from hic_genome_assembler_amd import _lib
    monkeypatch.setattr(_lib, "Context", NumpyContext)
    return _lib


def _case(name):
    """(map as loaded, bin IDs, scaffolds of the bins, groups of the golden file, {scaffold: bins in the bed})."""
    spec, _meta, _gold, lay, c = gc.load_case(name)
    bed = [(lay.scaffold_names[lay.scaffold_of_bin[k]], int(lay.bin_ids[k])) for k in range(lay.n_bins)]
    M, ids, scaffolds = ref.case_inputs(bed, c, [int(lay.bin_ids[b]) for b in spec.get("nan_bias", ())])
    groups = ref.read_group_file(os.path.join(gc.GOLDEN_DIR, name, "chromosomeGroups.txt"))
    return M, ids, scaffolds, groups, ref.scaffold_bin_counts(bed)


def _package_records(M, ids, scaffolds, groups, counts, min_ratio=3.0):
    from hic_genome_assembler_amd import scaffoldToChromosomes as p1
    from hic_genome_assembler_amd.hostio import Bin
    bins = [Bin(b, s, 0, 1, 1.0, 0.0) for b, s in zip(ids, scaffolds)]
    chroms = [[[int(ln.split("\t")[0]), ln.split("\t")[1]] for ln in lines] for _h, lines in groups]
    return p1.groupSupport(_Matrix(M), bins, chroms, counts, minRatio=min_ratio)


def _same_records(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        for key in ("scaffold", "bins", "live_bins", "assigned", "best", "best_density", "second", "second_density",
                    "ratio", "verdict", "runs", "live_ids", "density"):
            assert g[key] == e[key], (e["scaffold"], key, g[key], e[key])


def test_the_double_sums_in_the_definitions_order():
    M, ids, scaffolds, groups, counts = _case("n300_edges")
    sid = {s: k for k, s in enumerate(counts)}
    scaf = np.array([sid[s] for s in scaffolds])
    grp = ref.labels_of(groups, ids)
    ctx = NumpyContext()
    ctx.set_contacts(M)
    b, s = ctx.group_sums(grp, scaf, len(groups), len(counts))
    rb, rs = ref.group_sums(M, grp, scaf, len(groups), len(counts))
    assert np.array_equal(b, rb) and np.array_equal(s, rs)
    # the column form equals the row form on a symmetric map, up to the order of the additions
    g0 = np.flatnonzero(grp == 0)
    i = int(np.flatnonzero(grp == 1)[0])
    assert rb[i, 0] == pytest.approx(float(M[i, g0][scaf[g0] != scaf[i]].sum()), rel=1e-12)


@pytest.mark.parametrize("name", sorted(COUNTS))
def test_golden_group_files_verdict_counts(name):
    M, ids, scaffolds, groups, counts = _case(name)
    exp = ref.records(M, ids, scaffolds, groups, counts)
    print(name, "verdicts of the reference module:", ref.verdict_counts(exp))
    assert ref.verdict_counts(exp) == COUNTS[name]
    # L_s over all bins of a scaffold (the prototype's |s|) gives the same verdicts: zero rows do not move the counts
    alt = ref.records(M, ids, scaffolds, groups, counts, live_is_all=True)
    assert [r["verdict"] for r in alt] == [r["verdict"] for r in exp]
    got = _package_records(M, ids, scaffolds, groups, counts)
    _same_records(got, exp)
    assert [r["scaffold"] for r in got] == list(counts)


@pytest.mark.parametrize("name", LEAVE_OUT)
def test_leave_out_scaffolds_come_back_to_their_group(name):
    M, ids, scaffolds, groups, counts = _case(name)
    kept, gone = ref.withhold(groups, counts, step=5)
    exp = ref.records(M, ids, scaffolds, kept, counts, min_ratio=3.0)
    got = _package_records(M, ids, scaffolds, kept, counts, min_ratio=3.0)
    _same_records(got, exp)
    by_name = {r["scaffold"]: r for r in got}
    assert all(by_name[s]["assigned"] is None for s in gone)
    rescued = [s for s in gone if by_name[s]["verdict"] == "rescued"]
    wrong = [s for s in rescued if by_name[s]["best"] != gone[s]]
    print(name, "withheld %d, rescued %d, wrong %d" % (len(gone), len(rescued), len(wrong)))
    assert not wrong
    assert 2 * len(rescued) >= len(gone)


def _toy():
    """Two groups of 3 + 3 bins in scaffolds a (bins 1-3, group 1) and b (4-6, group 2); c (7, 8) is unassigned and touches
    group 2 three times as densely as group 1; d (9) touches both alike; e (10) has no contacts; f is only in the bed."""
    names = ["a"] * 3 + ["b"] * 3 + ["c"] * 2 + ["d", "e"]
    M = np.zeros((10, 10))
    M[0:3, 0:3] = 5.0
    M[3:6, 3:6] = 5.0
    M[0:3, 3:6] = M[3:6, 0:3] = 1.0
    for i in (6, 7):
        M[i, 0:3] = M[0:3, i] = 1.0
        M[i, 3:6] = M[3:6, i] = 3.0
    M[8, 0:6] = M[0:6, 8] = 2.0
    ids = list(range(1, 11))
    groups = [("### Chromosome group 1 ###", ["1\ta", "2\ta", "3\ta"]), ("### Chromosome group 2 ###", ["4\tb", "5\tb", "6\tb"])]
    counts = {"a": 3, "b": 3, "c": 2, "d": 1, "e": 1, "f": 4}
    return M, ids, names, groups, counts


def test_verdicts_and_report_text_of_a_toy_map(tmp_path):
    from hic_genome_assembler_amd import scaffoldToChromosomes as p1
    M, ids, names, groups, counts = _toy()
    got = _package_records(M, ids, names, groups, counts, min_ratio=3.0)
    _same_records(got, ref.records(M, ids, names, groups, counts, min_ratio=3.0))
    by = {r["scaffold"]: r for r in got}
    # a's own bins never vote for it: its only evidence for group 1 would be itself, so group 2 is denser
    assert by["a"]["density"] == [0.0, 1.0] and by["a"]["verdict"] == "contested"
    assert (by["c"]["verdict"], by["c"]["best"], by["c"]["second"], by["c"]["ratio"]) == ("rescued", 1, 0, 3.0)
    assert by["c"]["runs"] == "2:2" and by["c"]["live_ids"] == [7, 8]
    assert (by["d"]["verdict"], by["d"]["ratio"], by["d"]["best"]) == ("ambiguous", 1.0, 0)
    assert by["e"]["verdict"] == "no_contacts" and by["e"]["live_bins"] == 0 and by["e"]["runs"] == "NA"
    assert by["f"]["verdict"] == "no_contacts" and (by["f"]["bins"], by["f"]["live_bins"]) == (4, 0)
    # minRatio is the user's: at 3.5 c is no longer rescued
    assert {r["scaffold"]: r["verdict"] for r in _package_records(M, ids, names, groups, counts, min_ratio=3.5)}["c"] == "ambiguous"
    text = p1.groupSupportText(got)
    assert text == ref.report_text(got)
    lines = text.splitlines()
    assert lines[0] == "#scaffold\tbins\tlive_bins\tassigned\tbest\tbest_density\tsecond\tsecond_density\tratio\tverdict\truns"
    assert all(len(ln.split("\t")) == 11 for ln in lines)
    assert lines[3] == "c\t2\t2\tNA\t2\t3.0\t1\t1.0\t3.0\trescued\t2:2"
    assert lines[6] == "f\t4\t0\tNA\tNA\tNA\tNA\tNA\tNA\tno_contacts\tNA"
    # one group only: no second, ratio inf
    one = _package_records(M, ids, names, groups[:1], counts)
    c = {r["scaffold"]: r for r in one}["c"]
    assert (c["second"], c["ratio"], c["verdict"]) == (None, float("inf"), "rescued")
    assert p1.groupSupportText(one).splitlines()[3].split("\t")[6:9] == ["NA", "NA", "inf"]
    p1.writeGroupSupportToFile(got, str(tmp_path / "r.txt"), str(tmp_path / "full"))
    assert (tmp_path / "r.txt").read_text() == text
    full = (tmp_path / "full" / "groupSupport.full.tsv").read_text().splitlines()
    assert full[0] == "scaffold\tgroup1\tgroup2" and full[3] == "c\t1.0\t3.0" and len(full) == 7


def test_zero_rows_compacted_or_not_give_the_same_records():
    M, ids, names, groups, counts = _toy()
    full = _package_records(M, ids, names, groups, counts)
    keep = [k for k in range(10) if k != 9]                   # e's row is zero
    compacted = _package_records(M[np.ix_(keep, keep)], [ids[k] for k in keep], [names[k] for k in keep], groups, counts)
    _same_records(compacted, full)
    # a label on a zero row is ignored: the same records again
    labelled = [groups[0], (groups[1][0], groups[1][1] + ["10\te"])]
    a = _package_records(M, ids, names, labelled, counts)
    b = _package_records(M[np.ix_(keep, keep)], [ids[k] for k in keep], [names[k] for k in keep], labelled, counts)
    _same_records(a, b)
    assert {r["scaffold"]: r for r in a}["e"]["assigned"] is None


def test_rescued_file_round_trips_through_part2_readers(tmp_path):
    from hic_genome_assembler_amd import orderGenome as p2, scaffoldToChromosomes as p1
    M, ids, names, groups, counts = _toy()
    got = _package_records(M, ids, names, groups, counts)
    src = tmp_path / "groups.txt"
    src.write_text("".join(h + "\n" + "".join(ln + "\n" for ln in lines) for h, lines in groups))
    out = tmp_path / "rescued.txt"
    assert p1.writeRescuedGroupsToFile(got, str(src), str(out)) == 1
    assert out.read_text() == ref.rescued_text(got, groups)
    assert out.read_text() == "### Chromosome group 1 ###\n1\ta\n2\ta\n3\ta\n### Chromosome group 2 ###\n4\tb\n5\tb\n6\tb\n7\tc\n8\tc\n"
    assert p2.readChromsFromFile(str(out)) == [[[1, "a"], [2, "a"], [3, "a"]], [[4, "b"], [5, "b"], [6, "b"], [7, "c"], [8, "c"]]]
    assert sorted(p2.readGroupingsToValidBins(str(out))) == list(range(1, 9))
    assert src.read_text().count("\n") == 8                   # the input is never changed


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


def test_optional_config_lines_and_resolve(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run, supportPart1 as sp
    paths = {k: "x" for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    cfg, files = _config(tmp_path, paths)
    v = run.readConfigFileToVariables(cfg)
    assert "groupSupportFile" not in v and "rescuedChromosomeGroupFile" not in v      # absent lines: absent keys
    assert not run.ensureAllVariablesAreSet(v)
    args = sp._parse_args(["-config", cfg])
    assert args.minRatio == 3.0 and args.device == 0
    assert sp.resolve(args, v) == (files + "/chromosomeGroups.txt", os.path.join(files, "groupSupport.txt"), None)
    cfg, files = _config(tmp_path, paths, groupSupportFile="gs.txt", rescuedChromosomeGroupFile="rescued.txt")
    v = run.readConfigFileToVariables(cfg)
    assert v["groupSupportFile"] == files + "/gs.txt" and v["rescuedChromosomeGroupFile"] == files + "/rescued.txt"
    assert not run.ensureAllVariablesAreSet(v)
    assert sp.resolve(sp._parse_args(["-config", cfg]), v) == (files + "/chromosomeGroups.txt", files + "/gs.txt", files + "/rescued.txt")
    args = sp._parse_args(["-config", cfg, "-chromosomeGroupFile", "g", "-out", "o", "-rescued", "r", "-minRatio", "2.5",
                           "-full", "d", "-device", "1"])
    assert sp.resolve(args, v) == ("g", "o", "r") and (args.minRatio, args.full, args.device) == (2.5, "d", 1)


def test_command_line_from_files_on_n300_edges(fake_gpu, tmp_path):
    """supportPart1 on the golden group file of n300_edges (NaN-bias bins dropped by the loader, zero rows left in the
    map), with every 5th scaffold withheld so that the rescued file differs from its input."""
    from hic_genome_assembler_amd import orderGenome as p2, supportPart1 as sp
    name = "n300_edges"
    paths = gc.write_case_files(name, str(tmp_path))
    M, ids, scaffolds, groups, counts = _case(name)
    kept, gone = ref.withhold(groups, counts, step=5)
    cfg, files = _config(tmp_path, paths, groupSupportFile="gs.txt")
    with open(os.path.join(files, "chromosomeGroups.txt"), "w") as fh:
        fh.write("".join(h + "\n" + "".join(ln + "\n" for ln in lines) for h, lines in kept))
    sp.main(["-config", cfg, "-rescued", os.path.join(files, "rescued.txt"), "-full", os.path.join(files, "full")])
    exp = ref.records(M, ids, scaffolds, kept, counts)
    with open(os.path.join(files, "gs.txt")) as fh:
        assert fh.read() == ref.report_text(exp)
    with open(os.path.join(files, "rescued.txt")) as fh:
        text = fh.read()
    assert text == ref.rescued_text(exp, kept)
    rescued = [r for r in exp if r["verdict"] == "rescued"]
    assert rescued and all(r["scaffold"] in gone for r in rescued)
    chroms = p2.readChromsFromFile(os.path.join(files, "rescued.txt"))
    assert len(chroms) == len(kept)
    for r in rescued:
        assert [e[0] for e in chroms[r["best"]] if e[1] == r["scaffold"]] == r["live_ids"]
    assert os.path.exists(os.path.join(files, "full", "groupSupport.full.tsv"))
