"""Inversion support and the refinement (orderGenome.inversionSupport / refineOrdering, supportInversions.py,
refinePart2.py) on the CPU: the report text and the -full tables from a hand-made results dict, held to
tests/inversion_reference.py's restatements; the competing mask against bin orders compared as lists; the host
restatement of the device's pick; choose_move and apply_move; the command lines, the config keys and the C header."""
import itertools
import os

import numpy as np
import pytest

import golden_cases as gc
import inversion_reference as ref
from test_support_cpu import _config


def _hand_made():
    """Two chromosomes as inversion_reference describes them and as inversionSupport returns them: an invertible left
    end, a supported one, the last scaffold NA; a chromosome of two scaffolds, where nothing competes."""
    oracle = [dict(score0=1.25, names=["beta", "alpha", "gamma", "delta"], orientations=["+", "-", "+", "-"],
                   table=np.arange(16.0).reshape(4, 4) / 7.0,
                   rows={0: dict(bins=3, best=2, end="gamma", span=3, span_bins=8, delta=0.5, gain=0.4, verdict="invertible"),
                         1: dict(bins=4, best=3, end="delta", span=3, span_bins=7, delta=-0.125, gain=-0.1, verdict="supported"),
                         2: dict(bins=1, best=3, end="delta", span=2, span_bins=3, delta=0.0, gain=0.0, verdict="supported"),
                         3: dict(bins=2, best=None, verdict="NA")}),
              dict(score0=0.1 + 0.2, names=["alpha", "delta"], orientations=["+", "+"], table=np.array([[0.3, 0.3], [0.0, 0.25]]),
                   rows={0: dict(bins=2, best=None, verdict="NA"), 1: dict(bins=3, best=None, verdict="NA")})]
    product = []
    for res in oracle:
        rows = []
        for i in range(len(res["names"])):
            r = res["rows"][i]
            rows.append(dict(bins=r["bins"], best_j=r["best"], best_end=r.get("end"), span=r.get("span"),
                             span_bins=r.get("span_bins"), best_delta=r.get("delta"), gain=r.get("gain"), verdict=r["verdict"],
                             near=0 if r["best"] is None else 1))
        product.append(dict(score0=res["score0"], total=1.0, names=res["names"], orientations=res["orientations"], rows=rows,
                            table=res["table"], maxSpan=0))
    return oracle, product


def test_report_text_and_full_tables(tmp_path, capsys):
    from hic_genome_assembler_amd import orderGenome as p2
    oracle, product = _hand_made()
    text = p2.inversionSupportText(product)
    assert text == ref.report_text(oracle)
    lines = text.splitlines()
    assert lines[0] == "### Chromosome grouping 1 ### 1.25"
    assert lines[1] == "beta\t+\t3\tgamma\t3\t8\t0.5\t0.4\tinvertible"
    assert lines[2] == "alpha\t-\t4\tdelta\t3\t7\t-0.125\t-0.1\tsupported"
    assert lines[3] == "gamma\t+\t1\tdelta\t2\t3\t0.0\t0.0\tsupported"         # a zero delta is not an improvement
    assert lines[4] == "delta\t-\t2\tNA\tNA\tNA\tNA\tNA\tNA"
    assert lines[5] == "### Chromosome grouping 2 ### 0.30000000000000004"
    p2.writeInversionSupportToFile(product, str(tmp_path / "report.txt"), str(tmp_path / "full"))
    assert (tmp_path / "report.txt").read_text() == text
    for k, res in enumerate(oracle):
        assert (tmp_path / "full" / ("Chr_%d.inversions.tsv" % (k + 1))).read_text() == ref.full_text(res)
    full = (tmp_path / "full" / "Chr_1.inversions.tsv").read_text().splitlines()
    assert full[0].split("\t") == ["scaffold", "beta", "alpha", "gamma", "delta"]
    assert [float(v) for v in full[2].split("\t")[1:]] == list(oracle[0]["table"][1])
    assert "Inversion support written for scaffolds 6" in capsys.readouterr().out


def test_competing_mask_against_bin_orders_compared_as_lists():
    """Every S up to 6 and every pattern of one-bin and multi-bin scaffolds: a candidate competes when its segment has
    two scaffolds or more, its bin order is neither the arrangement's nor its mirror image nor an earlier candidate's of
    the same left end, and it is no wider than maxSpan.  _inversion_row against list slicing on the way."""
    from hic_genome_assembler_amd import orderGenome as p2

    class Layout:                                             # ChromosomeLayout's host side: ranges of a selection
        def __init__(self, lengths):
            self.length = list(lengths)
            self.start = [sum(lengths[:k]) for k in range(len(lengths))]
        positions = p2.ChromosomeLayout.positions
        node_row = p2.ChromosomeLayout.node_row

    for S in range(1, 7):
        for pattern in itertools.product((1, 3), repeat=S):
            layout = Layout(pattern)
            layout._pos_cache = {}
            ids = list(range(S))[::-1]                        # an arrangement that is not the layout order
            rev = [k % 2 for k in range(S)]
            laid = [list(layout.positions(i, r)) for i, r in zip(ids, rev)]
            row0 = [x for p in laid for x in p]
            for max_span in (0, 2, 3):
                mask = p2.inversion_counts(S, max_span)
                assert mask.shape == (S, S) and mask.dtype == bool
                for i in range(S):
                    seen = []
                    for j in range(S):
                        if j < i:
                            assert not mask[i, j]
                            continue
                        cand = [x for p in ref.inverted(laid, i, j, lambda p: p[::-1]) for x in p]
                        assert list(p2._inversion_row(layout, ids, rev, i, j)) == cand
                        new = j > i and cand != row0 and cand != row0[::-1] and cand not in seen
                        seen.append(cand)
                        assert bool(mask[i, j]) == (new and (max_span == 0 or j - i + 1 <= max_span)), (pattern, i, j, max_span)
    assert not p2.inversion_counts(2).any() and not p2.inversion_counts(1).any()
    assert p2.inversion_counts(3).tolist() == [[False, True, False], [False, False, True], [False, False, False]]


def test_work_count_against_a_double_loop():
    from hic_genome_assembler_amd import orderGenome as p2
    lengths = [3, 1, 4, 1, 5, 9]
    n = sum(lengths)
    for max_span in (0, 1, 2, 3, 7):
        want = 0
        for i in range(len(lengths)):
            for j in range(i, len(lengths)):
                if max_span == 0 or j - i + 1 <= max_span:
                    seg = sum(lengths[i:j + 1])
                    want += seg * (n - seg)
        assert p2.inversion_work(lengths, max_span) == want
    # the bench map's largest chromosome is far below the bound of a call, 4,096 scaffolds of 10 bins far above it
    assert p2.inversion_work([13] * 142) < 1e10 < 1e13 < p2.inversion_work([10] * 4096)
    assert p2.inversion_work([10] * 4096, 8) < 1e13


def test_summary_with_a_tie_a_nan_and_an_empty_row():
    from hic_genome_assembler_amd import orderGenome as p2
    t = np.zeros((5, 5))
    t[0] = [9.0, 5.0, 5.0, 5.0 * (1 - 5e-10), 99.0]           # the diagonal and (0, S - 1) never win; a tie: the first
    t[1] = [50.0, 7.0, np.nan, 3.0, 2.0]                      # left of the diagonal never; a NaN does not compete
    t[2] = [0.0, 0.0, 1.0, -4.0, -4.0 * (1 + 5e-10)]          # negative scores: the band is relative to |top|
    t[3] = [0.0, 0.0, 0.0, 2.0, np.nan]                       # only a NaN competes: nothing
    assert p2.inversion_summary(t).tolist() == [[1, 3], [3, 1], [3, 2], [-1, 0], [-1, 0]]
    assert p2.inversion_summary(t, 2).tolist() == [[1, 1], [-1, 0], [3, 1], [-1, 0], [-1, 0]]
    assert p2.inversion_summary(t, 3).tolist() == [[1, 2], [3, 1], [3, 2], [-1, 0], [-1, 0]]
    assert p2.inversion_summary(np.zeros((1, 1))).tolist() == [[-1, 0]]
    assert p2.inversion_summary(np.ones((2, 2))).tolist() == [[-1, 0], [-1, 0]]


def test_choose_move():
    from hic_genome_assembler_amd import orderGenome as p2
    rel = [None, (2, 1, 0.25), (0, 0, 0.5), (1, 0, 0.5)]
    inv = [(2, 0.5), (3, 0.75), None, None]
    assert p2.choose_move(rel, inv, 2.0) == ("invert", 1, 3, 0.75)
    # an exact tie between a relocation and an inversion goes to the relocation, and to the first of equal relocations
    assert p2.choose_move(rel, [(2, 0.5), None, None, None], 2.0) == ("relocate", 2, 0, 0, 0.5)
    assert p2.choose_move(None, inv, 2.0) == ("invert", 1, 3, 0.75)
    assert p2.choose_move(rel, None, 2.0) == ("relocate", 2, 0, 0, 0.5)
    # minGain is relative to |score0| and strict; a zero or negative delta means converged
    assert p2.choose_move(rel, inv, 2.0, minGain=0.3) == ("invert", 1, 3, 0.75)
    assert p2.choose_move(rel, inv, 2.0, minGain=0.375) is None
    assert p2.choose_move(rel, inv, -2.0, minGain=0.375) is None
    assert p2.choose_move([(1, 0, 0.0)], [None], 2.0) is None
    assert p2.choose_move([(1, 0, -1e-3), None], [(1, -1e-9), None], 2.0) is None
    assert p2.choose_move([None, None], [None, None], 2.0) is None
    assert p2.choose_move([], [], 0.0) is None


def test_apply_move_against_list_slicing():
    from hic_genome_assembler_amd import orderGenome as p2
    names = ["a", "b", "c", "d", "e"]
    arr = [("a", "+"), ("b", "-"), ("c", "+"), ("d", "-"), ("e", "+")]
    ids, rev = [4, 2, 0, 3, 1], [0, 1, 0, 1, 0]               # ids are layout ids, not positions
    as_arr = lambda i, r: [(names[[4, 2, 0, 3, 1].index(x)], "-" if y else "+") for x, y in zip(i, r)]
    assert as_arr(ids, rev) == arr
    for i in range(5):
        for j in range(i, 5):
            move = ("invert", i, j, 0.1)
            got = p2.apply_move(ids, rev, move)
            assert as_arr(*got) == ref.invert_arrangement(arr, i, j)
            assert p2.apply_move(*got, move) == (ids, rev)    # an inversion applied twice is the identity
    for j in range(5):
        for g in range(5):
            for r in (0, 1):
                got = p2.apply_move(np.array(ids, np.int32), np.array(rev, np.uint8), ("relocate", j, g, r, 0.1))
                assert as_arr(*got) == ref.relocate_arrangement(arr, j, g, "-" if r else "+")
    assert (ids, rev) == ([4, 2, 0, 3, 1], [0, 1, 0, 1, 0])   # the inputs are not changed
    with pytest.raises(ValueError):
        p2.apply_move(ids, rev, ("swap", 0, 1, 0.1))
    # Scaffold lists follow the same moves: bins reversed with every flip
    group = [p2.Scaffold(nm, [10 * k, 10 * k + 1], "+") for k, nm in enumerate(names)]
    group[1].flipOrientation()
    moved = p2._moved_group(group, ("invert", 0, 2, 0.1))
    assert [(s.name, s.orientation, s.binList) for s in moved[:3]] == [("c", "-", [21, 20]), ("b", "+", [10, 11]), ("a", "-", [1, 0])]
    moved = p2._moved_group(group, ("relocate", 1, 3, 1, 0.1))
    assert [(s.name, s.orientation) for s in moved] == [("a", "+"), ("c", "+"), ("d", "+"), ("b", "-"), ("e", "+")]
    assert moved[3].binList == [11, 10]
    moved = p2._moved_group(group, ("relocate", 1, 0, 0, 0.1))
    assert (moved[0].name, moved[0].orientation, moved[0].binList) == ("b", "+", [10, 11])
    assert (group[1].orientation, group[1].binList) == ("-", [11, 10])          # copies: the input is not changed


def test_refinement_files_from_a_hand_made_run(tmp_path, capsys):
    from hic_genome_assembler_amd import orderGenome as p2
    group = [p2.Scaffold("a", [1, 2], "+"), p2.Scaffold("b", [5], "+")]
    log = [dict(round=1, chromosome=1, kind="invert", scaffold="a..b", to="reversed", before=1.0, after=1.5),
           dict(round=2, chromosome=1, kind="relocate", scaffold="b", to="0-", before=1.5, after=1.75)]
    log[0]["from"], log[1]["from"] = "0..1", "1+"
    summary = [dict(before=1.0, after=1.75, moves=2, rounds=3, converged=True), dict(before=0.5, after=0.5, moves=0, rounds=1,
                                                                                      converged=False)]
    out = p2.writeRefinement([group, []], log, summary, str(tmp_path / "r"), "/x/orders.txt", "/y/plot.txt")
    assert out == str(tmp_path / "r" / "orders.txt")
    assert (tmp_path / "r" / "orders.txt").read_text() == "### Chromosome grouping 1 ###\na\t+\nb\t+\n### Chromosome grouping 2 ###\n"
    assert (tmp_path / "r" / "plot.txt").read_text() == "#ScaffoldID\tHiCPro-BinID\na\t1\na\t2\nb\t5"
    assert (tmp_path / "r" / "refine.log").read_text() == ("1\t1\tinvert\ta..b\t0..1 -> reversed\t1.0\t1.5\n"
                                                            "2\t1\trelocate\tb\t1+ -> 0-\t1.5\t1.75\n")
    assert (tmp_path / "r" / "refine_summary.tsv").read_text() == (
        "chromosome\tscore_before\tscore_after\tmoves\trounds\tconverged\n1\t1.0\t1.75\t2\t3\tyes\n2\t0.5\t0.5\t0\t1\tno\n")
    assert "Refinement moves applied 2" in capsys.readouterr().out
    with pytest.raises(ValueError):
        p2.refineOrdering(None, [], [], None, moves=("swap",))


def test_command_lines_and_config_handling(tmp_path):
    from hic_genome_assembler_amd import refinePart2 as rp, run_hicAssembler as run, supportInversions as si
    paths = gc.write_case_files("n160", str(tmp_path))
    cfg, files = _config(tmp_path, paths)
    v = run.readConfigFileToVariables(cfg)
    assert "inversionSupportFile" not in v and "refinedChromosomeOrderFile" not in v and not run.ensureAllVariablesAreSet(v)
    args = si._parse_args(["-config", cfg])
    assert (args.device, args.full, args.out, args.maxSpan, args.chromosomeOrderFile) == (0, None, None, 0, None)
    assert si.resolve(args, v) == (files + "/chromosomeOrders.txt", os.path.join(files, "inversionSupport.txt"))
    args = si._parse_args(["-config", cfg, "-chromosomeOrderFile", "ref.txt", "-out", "o.txt", "-maxSpan", "12", "-full", "d",
                           "-device", "2"])
    assert si.resolve(args, v) == ("ref.txt", "o.txt") and (args.full, args.device, args.maxSpan) == ("d", 2, 12)
    cfg2, files = _config(tmp_path, paths, inversionSupportFile="inv.txt", refinedChromosomeOrderFile="refined.txt")
    v2 = run.readConfigFileToVariables(cfg2)
    assert v2["inversionSupportFile"] == files + "/inv.txt" and v2["refinedChromosomeOrderFile"] == files + "/refined.txt"
    assert not run.ensureAllVariablesAreSet(v2)
    assert si.resolve(si._parse_args(["-config", cfg2]), v2)[1] == files + "/inv.txt"
    assert {k: x for k, x in v2.items() if k not in ("inversionSupportFile", "refinedChromosomeOrderFile")} == v
    # refinePart2
    args = rp._parse_args(["-config", cfg])
    assert (args.moves, args.maxSpan, args.minGain, args.maxRounds, args.device, args.out) == ("relocate,invert", 0, 0.0, 100, 0, None)
    assert rp.resolve(args, v) == (files + "/chromosomeOrders.txt", os.path.join(files, "refined"), ("relocate", "invert"))
    args = rp._parse_args(["-config", cfg, "-chromosomeOrderFile", "ref.txt", "-out", "d", "-moves", "invert", "-maxSpan", "12",
                           "-minGain", "1e-4", "-maxRounds", "7", "-device", "1"])
    assert rp.resolve(args, v) == ("ref.txt", "d", ("invert",))
    assert (args.maxSpan, args.minGain, args.maxRounds, args.device) == (12, 1e-4, 7, 1)
    assert rp.parse_moves("invert, relocate") == ("relocate", "invert") and rp.parse_moves("relocate") == ("relocate",)
    # refusals: an unknown family, an empty list, negative or zero limits, no config; and the input is never the output
    for bad in ("swap", "", "relocate,swap"):
        with pytest.raises(ValueError):
            rp.parse_moves(bad)
        with pytest.raises(SystemExit):
            rp.main(["-config", cfg, "-moves", bad])
    for extra in (["-maxRounds", "0"], ["-maxSpan", "-1"], ["-minGain", "-0.5"]):
        with pytest.raises(SystemExit):
            rp.main(["-config", cfg] + extra)
    with pytest.raises(SystemExit):
        si.main(["-config", cfg, "-maxSpan", "-1"])
    for mod in (si, rp):
        with pytest.raises(SystemExit):
            mod._parse_args([])
    with pytest.raises(ValueError):
        rp.runRefine("bed", "bias", "matrix", "groups", str(tmp_path / "d" / "orders.txt"), "plot.txt", str(tmp_path / "d"))


def test_the_header_declares_the_two_exports(repo_root):
    with open(os.path.join(repo_root, "include", "hicmi.h")) as fh:
        header = fh.read()
    assert ("int hicmi_p2_inversions(hicmi_ctx *ctx, const int32_t *ids, const uint8_t *rev, int64_t S, double total, "
            "int64_t max_span") in header
    assert "int hicmi_p2_inversions_multi(int64_t n_jobs, hicmi_ctx *const *ctxs" in header
    from hic_genome_assembler_amd import _lib
    assert {"hicmi_p2_inversions", "hicmi_p2_inversions_multi"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["hicmi_p2_inversions_multi"][1]) == 9 and len(_lib.SIGNATURES["hicmi_p2_inversions"][1]) == 8
