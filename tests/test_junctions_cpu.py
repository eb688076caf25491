"""Junction support (orderGenome.junctionSupport and its pure parts, supportJunctions.py) on the CPU: the
records and norms against index arrays and a double loop; junction_summary's tie rules and NA cases on hand-made sums;
join_chromosomes and cut_chromosomes against tests/junction_reference.py's plain-list restatements and by hand; the host
flow, the report and the three files on n160 with the NumPy context standing in for the device; the command line, the
config keys, the C header and the binding."""
import contextlib
import io
import itertools
import os

import numpy as np
import pytest

import golden_cases as gc
import junction_reference as ref
from support_reference import read_group_file, read_order_file
from test_support_cpu import _config


def _sides(records, bins):
    """Every record's two sides as explicit lists of ``bins`` entries."""
    out = []
    for sa, ta, la, sb, tb, lb in records["rec"].tolist():
        out.append(([bins[sa + ta * k] for k in range(la)], [bins[sb + tb * k] for k in range(lb)]))
    return out


@pytest.mark.parametrize("window", [0, 1, 16])
def test_records_against_sides_built_from_lists(window):
    from hic_genome_assembler_amd import orderGenome as p2
    # chromosomes of 40 bins (longer than the window), 5 (shorter), 1 (one bin, one scaffold) and 17 with one-bin scaffolds
    scaffolds = [[7, 20, 1, 12], [2, 3], [1], [1, 15, 1]]
    lengths = [sum(s) for s in scaffolds]
    bounds = [list(np.cumsum(s)[:-1]) for s in scaffolds]
    records = p2.junction_records(lengths, bounds, window)
    bins = list(range(1000, 1000 + sum(lengths)))              # any labels: the records index the list
    chroms, at = [], 0
    for n in lengths:
        chroms.append(bins[at:at + n])
        at += n
    take = (lambda v: v[:window]) if window else (lambda v: v)
    want, internal = [], []
    for c, (chrom, bs) in enumerate(zip(chroms, bounds)):
        for k, p in enumerate(bs):
            want.append((take(chrom[:p][::-1]), take(chrom[p:])))
            internal.append((c, k))
    ends = [side for chrom in chroms for side in (take(chrom), take(chrom[::-1]))]
    pairs = [(e, f) for e, f in itertools.combinations(range(8), 2) if e // 2 != f // 2]
    want += [(ends[e], ends[f]) for e, f in pairs]
    assert _sides(records, bins) == want
    assert records["internal"] == internal and records["pairs"] == pairs and records["G"] == 4
    assert records["rec"].dtype == np.int64 and records["rec"].shape == (len(want), 6)
    assert set(records["rec"][:, 1].tolist()) | set(records["rec"][:, 4].tolist()) == {1, -1}
    if window == 1:
        assert set(records["rec"][:, 2].tolist()) == {1} and set(records["rec"][:, 5].tolist()) == {1}


def test_records_refuse_what_has_no_sides():
    from hic_genome_assembler_amd import orderGenome as p2
    for lengths, bounds, window in (([5], [[0]], 16), ([5], [[5]], 16), ([5], [[2, 2]], 16), ([5], [[3, 2]], 16),
                                    ([0], [[]], 16), ([5], [[]], -1)):
        with pytest.raises(ValueError):
            p2.junction_records(lengths, bounds, window)
    one = p2.junction_records([3], [[]], 16)                   # one chromosome of one scaffold: nothing to measure
    assert one["rec"].shape == (0, 6) and one["pairs"] == [] and one["internal"] == []


def test_norm_against_a_double_loop():
    from hic_genome_assembler_amd import orderGenome as p2
    for la, lb in [(1, 1), (1, 16), (16, 1), (16, 16), (3, 7), (40, 5), (5, 40), (65, 64), (257, 300)]:
        cnt = {}
        for a in range(la):
            for b in range(lb):
                cnt[a + b + 1] = cnt.get(a + b + 1, 0) + 1
        acc = 0.0
        for d in sorted(cnt):
            acc += cnt[d] * (1.0 / d)
        assert p2.junction_norm(la, lb) == acc == ref.norm(la, lb)
    assert p2.junction_norm(1, 1) == 1.0
    # a map of ones has J = 1: the weights of a record add up to its norm
    assert ref.side_sum(np.ones((30, 30)), list(range(12)), list(range(12, 30))) == pytest.approx(p2.junction_norm(12, 18), rel=1e-14)


def _summary(table_J, internal_J, lengths=None, window=1, minRel=0.25):
    """junction_summary on hand-made J: with window 1 every norm is 1.0, so the sums ARE the J."""
    from hic_genome_assembler_amd import orderGenome as p2
    G = len(table_J) // 2
    lengths = lengths or [len(x) + 1 for x in internal_J]
    records = p2.junction_records(lengths, [list(range(1, n)) for n in lengths], window)
    assert [len([1 for c, _k in records["internal"] if c == g]) for g in range(G)] == [len(x) for x in internal_J]
    sums = [v for x in internal_J for v in x] + [table_J[e][f] for e, f in records["pairs"]]
    return p2.junction_summary(np.array(sums, dtype=np.float64), records, minRel)


def test_summary_picks_the_first_maximum_and_tells_mutual_from_one_sided():
    T = np.zeros((6, 6))

    def put(e, f, v):
        T[e, f] = T[f, e] = v
    put(1, 2, 8.0)      # 1.tail - 2.head: mutual, strong
    put(3, 4, 8.0)      # 2.tail - 3.head: a tie in row 3 with ...
    put(3, 5, 8.0)      # ... 2.tail - 3.tail: the first maximum (end 4) wins
    put(0, 2, 0.5)
    put(0, 5, 0.5)      # row 0: a tie of two weak partners, the first (end 2) wins; not mutual
    res = _summary(T, [[4.0, 8.0, 2.0], [4.0], []])             # median of (4, 8, 2, 4) = 4.0
    assert res["ref"] == 4.0
    ends = res["ends"]
    assert [r["best"] for r in ends] == [2, 2, 1, 4, 3, 3]
    assert [r["mutual"] for r in ends] == [False, True, True, True, True, False]
    assert [r["verdict"] for r in ends] == ["free", "joinable", "joinable", "joinable", "joinable", "free"]
    assert res["joinable"] == [(1, 2, 8.0), (3, 4, 8.0)]
    assert ends[1]["rel"] == 2.0 and ends[0]["rel"] == 0.125 and ends[5]["J"] == 8.0
    # second: the best end of a chromosome other than best's (and the end's own); first maximum again
    assert [r["second"] for r in ends] == [5, 4, 4, 0, 0, 0]
    assert ends[0]["second_J"] == 0.5 and ends[1]["second_J"] == 0.0
    # internal verdicts: rel >= minRel holds, the bound included
    assert [r["verdict"] for r in res["internal"]] == ["held", "held", "held", "held"]
    res = _summary(T, [[4.0, 8.0, 1.0], [4.0], []])
    assert [r["verdict"] for r in res["internal"]] == ["held", "held", "held", "held"] and res["internal"][2]["rel"] == 0.25
    res = _summary(T, [[4.0, 8.0, 0.9], [4.0], []])
    assert [r["verdict"] for r in res["internal"]] == ["held", "held", "weak", "held"] and res["weak"] == [(0, 2)]
    assert np.array_equal(res["table"], res["table"].T, equal_nan=True)
    assert all(np.isnan(res["table"][e, e]) and np.isnan(res["table"][e, e ^ 1]) for e in range(6))
    # a mutual pair below minRel is free
    res = _summary(T, [[64.0, 64.0, 64.0], [64.0], []])
    assert res["joinable"] == [] and [r["verdict"] for r in res["ends"]] == ["free"] * 6 and res["ends"][1]["mutual"]


def test_summary_na_cases():
    T2 = np.array([[0, 0, 3.0, 1.0], [0, 0, 2.0, 5.0], [3.0, 2.0, 0, 0], [1.0, 5.0, 0, 0]])
    res = _summary(T2, [[2.0], []])                              # G = 2: no second
    assert [r["second"] for r in res["ends"]] == [None] * 4 and [r["second_J"] for r in res["ends"]] == [None] * 4
    assert [r["best"] for r in res["ends"]] == [2, 3, 0, 1] and res["joinable"] == [(0, 2, 3.0), (1, 3, 5.0)]
    res = _summary(T2, [[], []], lengths=[1, 1])                 # no internal junction: no ref, no rel, no verdict
    assert res["ref"] is None and res["internal"] == []
    assert [r["best"] for r in res["ends"]] == [2, 3, 0, 1] and [r["J"] for r in res["ends"]] == [3.0, 5.0, 3.0, 5.0]
    assert all(r["rel"] is None and r["verdict"] is None for r in res["ends"]) and res["joinable"] == []
    res = _summary(T2, [[0.0, 0.0, 5.0], []])                    # ref = 0
    assert res["ref"] is None and all(r["verdict"] is None and r["rel"] is None for r in res["internal"])
    assert res["weak"] == [] and res["joinable"] == []
    res = _summary(np.zeros((2, 2)), [[2.0, 6.0]])               # G = 1: the ends have no partner
    assert res["ref"] == 4.0 and [r["verdict"] for r in res["internal"]] == ["held", "held"]
    assert all(r[k] is None for r in res["ends"] for k in ("best", "J", "rel", "mutual", "second", "second_J", "verdict"))
    assert [r["bins"] for r in res["ends"]] == [1, 1]


CHROMS = [[("a1", "+"), ("a2", "-")], [("b1", "+")], [("c1", "-"), ("c2", "+"), ("c3", "+")], [("d1", "+"), ("d2", "+")]]


def _as_ref(joins):
    return [((e // 2, e % 2), (f // 2, f % 2), J) for e, f, J in joins]


def test_join_a_path_entered_through_tails():
    from hic_genome_assembler_amd import orderGenome as p2
    # chromosome 3's tail on chromosome 1's head, chromosome 4's tail on chromosome 3's head... read so that 1 stays as written
    joins = [(0, 5, 3.0), (4, 7, 2.0)]
    got, members, applied, dropped = p2.join_chromosomes(CHROMS, joins)
    assert got == [[("d1", "+"), ("d2", "+"), ("c1", "-"), ("c2", "+"), ("c3", "+"), ("a1", "+"), ("a2", "-")], [("b1", "+")]]
    assert members == [[(3, False), (2, False), (0, False)], [(1, False)]] and applied == joins and dropped == []
    # tail to tail: the member entered through its tail is reversed, scaffold order and every orientation
    joins = [(1, 5, 3.0), (3, 4, 1.0)]
    got, members, applied, dropped = p2.join_chromosomes(CHROMS, joins)
    assert got == [[("a1", "+"), ("a2", "-"), ("c3", "-"), ("c2", "-"), ("c1", "+"), ("b1", "-")], [("d1", "+"), ("d2", "+")]]
    assert members == [[(0, False), (2, True), (1, True)], [(3, False)]]
    # head to head: the lowest-numbered member stays as written, so the OTHER one is read backwards, in front of it
    got, members, _a, _d = p2.join_chromosomes(CHROMS, [(2, 6, 1.0)])
    assert got == [CHROMS[0], [("d2", "-"), ("d1", "-"), ("b1", "+")], CHROMS[2]]
    assert members == [[(0, False)], [(3, True), (1, False)], [(2, False)]]
    for j in ([(1, 5, 3.0), (3, 4, 1.0)], [(0, 5, 3.0), (4, 7, 2.0)], [(2, 6, 1.0)], [(0, 2, 1.0), (1, 4, 1.0), (5, 7, 1.0)]):
        mine = p2.join_chromosomes(CHROMS, j)
        theirs = ref.join_plain(CHROMS, _as_ref(j))
        assert mine[0] == theirs[0] and mine[1] == theirs[1]


def test_join_a_cycle_drops_its_smallest_join_and_no_joins_change_nothing():
    from hic_genome_assembler_amd import orderGenome as p2
    got, members, applied, dropped = p2.join_chromosomes(CHROMS, [])
    assert got == CHROMS and members == [[(c, False)] for c in range(4)] and applied == [] and dropped == []
    cycle = [(1, 2, 5.0), (3, 4, 2.0), (0, 5, 4.0)]            # 1 -> 2 -> 3 -> back to 1: the 2.0 goes
    got, members, applied, dropped = p2.join_chromosomes(CHROMS, cycle)
    assert dropped == [(3, 4, 2.0)] and applied == [(1, 2, 5.0), (0, 5, 4.0)]
    assert got == [CHROMS[2] + CHROMS[0] + CHROMS[1], CHROMS[3]]
    tie = [(1, 2, 2.0), (3, 4, 2.0), (0, 5, 2.0)]              # a tie: the first listed goes
    got, members, applied, dropped = p2.join_chromosomes(CHROMS, tie)
    assert dropped == [(1, 2, 2.0)] and got == [CHROMS[1] + CHROMS[2] + CHROMS[0], CHROMS[3]]
    two = [(0, 3, 1.0), (1, 2, 7.0)]                            # a cycle of two chromosomes
    got, members, applied, dropped = p2.join_chromosomes(CHROMS, two)
    assert dropped == [(0, 3, 1.0)] and got == [CHROMS[0] + CHROMS[1], CHROMS[2], CHROMS[3]]
    for j in (cycle, tie, two):
        mine = p2.join_chromosomes(CHROMS, j)
        theirs = ref.join_plain(CHROMS, _as_ref(j))
        assert mine[0] == theirs[0] and mine[1] == theirs[1] and _as_ref(mine[3]) == theirs[2]
    for bad in ([(0, 1, 1.0)], [(0, 2, 1.0), (0, 4, 1.0)], [(0, 8, 1.0)]):
        with pytest.raises(ValueError):
            p2.join_chromosomes(CHROMS, bad)


def test_join_on_random_matchings_against_the_plain_lists():
    from hic_genome_assembler_amd import orderGenome as p2
    rng = np.random.default_rng(5)
    for _ in range(300):
        G = int(rng.integers(2, 8))
        chroms = [[("s%d_%d" % (c, k), "+-"[int(rng.integers(2))]) for k in range(int(rng.integers(1, 4)))] for c in range(G)]
        ends = [int(e) for e in rng.permutation(2 * G)]
        joins = []
        while len(ends) >= 2 and rng.random() < 0.8:
            e, f = ends.pop(), ends.pop()
            if e // 2 != f // 2:
                joins.append((min(e, f), max(e, f), float(rng.integers(1, 4))))
        mine = p2.join_chromosomes(chroms, joins)
        theirs = ref.join_plain(chroms, _as_ref(joins))
        assert mine[0] == theirs[0] and mine[1] == theirs[1] and _as_ref(mine[3]) == theirs[2], joins
        assert sorted(n for ch in mine[0] for n, _o in ch) == sorted(n for ch in chroms for n, _o in ch)


def test_cut_chromosomes():
    from hic_genome_assembler_amd import orderGenome as p2
    got, members = p2.cut_chromosomes(CHROMS, [])
    assert got == CHROMS and members == [(0, 0, 2), (1, 0, 1), (2, 0, 3), (3, 0, 2)]
    got, members = p2.cut_chromosomes(CHROMS, [(2, 1), (0, 0), (2, 0)])
    assert got == [[("a1", "+")], [("a2", "-")], [("b1", "+")], [("c1", "-")], [("c2", "+")], [("c3", "+")], CHROMS[3]]
    assert members == [(0, 0, 1), (0, 1, 2), (1, 0, 1), (2, 0, 1), (2, 1, 2), (2, 2, 3), (3, 0, 2)]
    assert got == ref.cut_plain(CHROMS, [(2, 1), (0, 0), (2, 0)])
    for bad in ([(1, 0)], [(0, 1)], [(4, 0)], [(0, -1)]):
        with pytest.raises(ValueError):
            p2.cut_chromosomes(CHROMS, bad)


# ---- the host flow on n160, the NumPy context standing in for the device --------------------------------
class _Bin:
    def __init__(self, ID):
        self.ID = ID


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _n160(groups=None, orders=None, **kw):
    from hic_genome_assembler_amd import orderGenome as p2
    name = "n160"
    lay, c = gc.load_case(name)[3:5]
    groups = groups or os.path.join(gc.GOLDEN_DIR, name, "chromosomeGroups.txt")
    orders = orders or os.path.join(gc.GOLDEN_DIR, name, "chromosomeOrders.txt")
    binList = [_Bin(int(b)) for b in lay.bin_ids]
    matrix = p2.GenomeMatrix(ref.NumpyJunctionContext(c))
    chromList = _quiet(p2.readChromsFromFile, groups)
    ordered = p2.scaffoldsFromOrderFile(chromList, orders)
    where = {int(b): i for i, b in enumerate(lay.bin_ids)}
    chroms = [ref.chromosome_sides(rows, arr, where) for rows, arr in zip(read_group_file(groups), read_order_file(orders))]
    return p2, matrix, ordered, binList, c, chroms


@pytest.mark.parametrize("window", [16, 0, 3])
def test_host_flow_and_report_text_on_n160(window, tmp_path, capsys):
    p2, matrix, ordered, binList, c, chroms = _n160()
    res = p2.junctionSupport(matrix, ordered, binList, window=window)
    exp = ref.analyse(c, chroms, window)
    assert np.array_equal(res["sums"], exp["sums"])             # the same NumPy sums: the host side adds nothing
    assert p2.junctionSupportText(res) == ref.report_text(exp)
    text = p2.junctionSupportText(res).splitlines()
    assert text[0] == "### reference %r window %d minRel 0.25" % (exp["ref"], window)
    assert text.count("### Chromosome ends ###") == 1 and len(text) == 1 + 4 + 26 + 1 + 8
    assert all(len(ln.split("\t")) == 7 for ln in text[1:31] if not ln.startswith("#"))
    assert all(len(ln.split("\t")) == 12 for ln in text[-8:])
    p2.writeJunctionSupportToFile(res, str(tmp_path / "j.txt"), str(tmp_path / "full"))
    assert "Junction support written for junctions 26 and chromosome ends 8" in capsys.readouterr().out
    with open(str(tmp_path / "j.txt")) as fh:
        assert fh.read() == ref.report_text(exp)
    with open(str(tmp_path / "full" / "junctions.ends.tsv")) as fh:
        full = [ln.split("\t") for ln in fh.read().splitlines()]
    assert full[0] == ["end", "1.head", "1.tail", "2.head", "2.tail", "3.head", "3.tail", "4.head", "4.tail"]
    assert full[1][1:3] == ["NA", "NA"] and float(full[1][3]) == exp["table"][0, 2] and full[8][0] == "4.tail"


def test_round_trips_on_n160_with_the_numpy_context(tmp_path):
    """The GPU suite's round trips (tests/test_gpu_junctions.py) with the sums from NumPy: a split chromosome comes back
    through writeJoinedFiles, two concatenated ones through writeCutFiles, the inputs untouched."""
    from test_gpu_junctions import concatenated_inputs, split_inputs
    name = "n160"
    gdir = os.path.join(gc.GOLDEN_DIR, name)
    groups, orders = os.path.join(gdir, "chromosomeGroups.txt"), os.path.join(gdir, "chromosomeOrders.txt")
    for chrom, swap in ((0, False), (3, True)):
        g2, o2 = split_inputs(str(tmp_path / ("split%d" % chrom)), groups, orders, chrom, swap)
        before = open(g2).read(), open(o2).read()
        p2, matrix, ordered, binList, _c, _chroms = _n160(g2, o2)
        res = p2.junctionSupport(matrix, ordered, binList)
        pair = (2 * chrom, 2 * chrom + 3) if swap else (2 * chrom + 1, 2 * chrom + 2)
        assert [(e, f) for e, f, _J in res["joinable"]] == [pair] and not res["weak"]
        out = str(tmp_path / ("joined%d" % chrom))
        new = _quiet(p2.writeJoinedFiles, res, ordered, out, g2, o2, str(tmp_path / "plotOrder.txt"))
        assert len(new) == 4
        for fn in ("chromosomeOrders.txt", "plotOrder.txt") + (("chromosomeGroups.txt",) if swap else ()):
            with open(os.path.join(out, fn)) as fh:
                assert fh.read() == gc.golden_text(name, fn), fn
        assert [sorted(map(tuple, g)) for g in read_group_file(os.path.join(out, "chromosomeGroups.txt"))] == \
            [sorted(map(tuple, g)) for g in read_group_file(groups)]
        with open(os.path.join(out, "joins.log")) as fh:
            log = fh.read().splitlines()
        assert len(log) == 1 and log[0].split("\t")[:5] == ["joined", str(pair[0] // 2 + 1), "head" if swap else "tail",
                                                            str(pair[1] // 2 + 1), "tail" if swap else "head"]
        assert (open(g2).read(), open(o2).read()) == before
        with pytest.raises(ValueError):                         # never over the input files
            p2.writeJoinedFiles(res, ordered, os.path.dirname(g2), g2, o2, str(tmp_path / "plotOrder.txt"))
    g2, o2, at = concatenated_inputs(str(tmp_path / "cat"), groups, orders)
    p2, matrix, ordered, binList, _c, _chroms = _n160(g2, o2)
    res = p2.junctionSupport(matrix, ordered, binList)
    assert res["weak"] == [(0, at)] and not res["joinable"]
    weak = [r for r in res["internal"] if r["verdict"] == "weak"]
    assert len(weak) == 1 and weak[0]["rel"] < 0.01
    out = str(tmp_path / "cut")
    _quiet(p2.writeCutFiles, res, ordered, out, g2, o2, str(tmp_path / "plotOrder.txt"))
    for fn in ("chromosomeOrders.txt", "plotOrder.txt", "chromosomeGroups.txt"):
        with open(os.path.join(out, fn)) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn
    with open(os.path.join(out, "cuts.log")) as fh:
        assert fh.read().split("\t")[:3] == ["1", ordered[0][at].name, ordered[0][at + 1].name]
    with pytest.raises(ValueError):                             # joins and cuts are never applied in one directory
        p2.junctionSupportToFiles(matrix, ordered, binList, g2, o2, "p.txt", None, out, out)


def test_command_line_and_config_handling(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run, supportJunctions as sj
    paths = gc.write_case_files("n160", str(tmp_path))
    cfg, files = _config(tmp_path, paths)
    v = run.readConfigFileToVariables(cfg)
    assert "junctionSupportFile" not in v and "joinedFilesDirectory" not in v and not run.ensureAllVariablesAreSet(v)
    args = sj._parse_args(["-config", cfg])
    assert (args.device, args.full, args.out, args.window, args.minRel, args.joined, args.cut, args.chromosomeOrderFile) == \
        (0, None, None, 16, 0.25, None, None, None)
    assert sj.resolve(args, v) == (files + "/chromosomeOrders.txt", os.path.join(files, "junctionSupport.txt"))
    args = sj._parse_args(["-config", cfg, "-chromosomeOrderFile", "ref.txt", "-out", "o.txt", "-window", "0", "-minRel", "0.5",
                           "-joined", "j", "-cut", "c", "-full", "d", "-device", "2"])
    assert sj.resolve(args, v) == ("ref.txt", "o.txt")
    assert (args.window, args.minRel, args.joined, args.cut, args.full, args.device) == (0, 0.5, "j", "c", "d", 2)
    cfg2, files = _config(tmp_path, paths, junctionSupportFile="junctions.txt", joinedFilesDirectory="joined")
    v2 = run.readConfigFileToVariables(cfg2)
    assert v2["junctionSupportFile"] == files + "/junctions.txt" and v2["joinedFilesDirectory"] == files + "/joined"
    assert not run.ensureAllVariablesAreSet(v2)
    assert sj.resolve(sj._parse_args(["-config", cfg2]), v2)[1] == files + "/junctions.txt"
    assert {k: x for k, x in v2.items() if k not in ("junctionSupportFile", "joinedFilesDirectory")} == v
    for extra in (["-window", "-1"], ["-minRel", "0"], ["-minRel", "-0.1"], ["-joined", "d", "-cut", "d"]):
        with pytest.raises(SystemExit):
            sj.main(["-config", cfg] + extra)
    with pytest.raises(SystemExit):
        sj._parse_args([])


def test_the_header_and_the_binding_declare_the_export(repo_root):
    with open(os.path.join(repo_root, "include", "hicmi.h")) as fh:
        header = fh.read()
    assert ("int hicmi_junction_sums(hicmi_ctx *ctx, const int32_t *bins, int64_t n_listed, const int64_t *rec, "
            "int64_t n_rec,\n                        double *sums_out);") in header
    assert "OG:608-612" in header[header.index("junction support"):header.index("int hicmi_junction_sums(")]
    from hic_genome_assembler_amd import _lib
    assert len(_lib.SIGNATURES["hicmi_junction_sums"][1]) == 6 and callable(_lib.Context.junction_sums)
