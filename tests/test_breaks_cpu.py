"""Break support (orderGenome.breakSupport, supportBreaks.py) on the CPU: the report text and the broken
group file from a hand-made results dict, held to tests/break_reference.py's restatements; the competing mask against
bin orders compared as lists; the command line, the config keys and the C header."""
import os

import numpy as np
import pytest

import break_reference as ref
import golden_cases as gc
from test_support_cpu import _config

GROUPS = ("### Chromosome group 1 ###\n7\talpha\n8\talpha\n9\talpha\n10\talpha\n3\tbeta\n4\tbeta\n5\tbeta\n20\tgamma\n"
          "### Chromosome group 2 ###\n30\tdelta\textra column\n31\tdelta\textra column\n32\tdelta\textra column\n41\talpha\n42\talpha\n")


def _hand_made():
    """Two chromosomes as break_reference describes them and as breakSupport returns them: a breakable '-' scaffold,
    an intact one, a one-bin NA; a breakable scaffold beside one that shares a name with chromosome 1 and is intact."""
    oracle = [dict(score0=1.25, names=["beta", "alpha", "gamma"], orientations=["+", "-", "+"],
                   rows={0: dict(bins=3, best=(1, 1, -0.125), cut=1, after=3, move="flip_right", delta=-0.125, gain=-0.1,
                                 verdict="intact"),
                         1: dict(bins=4, best=(1, 2, 0.5), cut=3, after=9, move="flip_left", delta=0.5, gain=0.4,
                                 verdict="breakable"),
                         2: dict(bins=1, best=None, verdict="NA")}),
              dict(score0=0.1 + 0.2, names=["alpha", "delta"], orientations=["+", "+"],
                   rows={0: dict(bins=2, best=None, verdict="NA"),
                         1: dict(bins=3, best=(2, 4, 1e-05), cut=2, after=31, move="swap", delta=1e-05, gain=1e-05 / (0.1 + 0.2),
                                 verdict="breakable")})]
    product = []
    for res in oracle:
        rows = []
        for j in range(len(res["names"])):
            r = res["rows"][j]
            rows.append(dict(bins=r["bins"], best_cut=r.get("cut"), cut_after_bin=r.get("after"), best_move=r.get("move"),
                             best_delta=r.get("delta"), gain=r.get("gain"), verdict=r["verdict"]))
        lengths = [r["bins"] for r in rows]
        n_rows = sum(max(ln - 1, 0) for ln in lengths)
        product.append(dict(score0=res["score0"], total=1.0, names=res["names"], orientations=res["orientations"], rows=rows,
                            table=np.arange(8.0 * n_rows).reshape(n_rows, 8) / 7.0,
                            offsets=[sum(max(ln - 1, 0) for ln in lengths[:j]) for j in range(len(lengths))], minPiece=1))
    return oracle, product


def test_report_text_and_broken_group_file(tmp_path, capsys):
    from hic_genome_assembler_amd import orderGenome as p2
    oracle, product = _hand_made()
    text = p2.breakSupportText(product)
    assert text == ref.report_text(oracle)
    assert text.splitlines()[2] == "alpha\t-\t4\t3\t9\tflip_left\t0.5\t0.4\tbreakable"
    assert text.splitlines()[3] == "gamma\t+\t1\tNA\tNA\tNA\tNA\tNA\tNA"
    assert text.splitlines()[4] == "### Chromosome grouping 2 ### 0.30000000000000004"
    groups = tmp_path / "groups.txt"
    groups.write_text(GROUPS)
    p2.writeBreakSupportToFile(product, str(tmp_path / "report.txt"), str(tmp_path / "full"))
    p2.writeBrokenGroupFile(product, str(groups), str(tmp_path / "broken.txt"))
    assert (tmp_path / "report.txt").read_text() == text
    broken = (tmp_path / "broken.txt").read_text()
    assert broken == ref.broken_text(oracle, GROUPS)
    assert groups.read_text() == GROUPS                               # the input is only read
    lines = broken.splitlines()
    assert lines[1:5] == ["7\talpha.brk1", "8\talpha.brk1", "9\talpha.brk1", "10\talpha.brk2"]
    assert lines[5:9] == GROUPS.splitlines()[5:9]                     # intact and NA scaffolds: verbatim
    assert lines[10:] == ["30\tdelta.brk1\textra column", "31\tdelta.brk1\textra column", "32\tdelta.brk2\textra column",
                          "41\talpha", "42\talpha"]                   # chromosome 2's alpha is not chromosome 1's
    with pytest.raises(ValueError):
        p2.writeBrokenGroupFile(product, str(groups), str(groups))
    # -full: one line per (scaffold, cut) in enumeration order; the cut is counted in the scaffold's own '+' direction
    full = (tmp_path / "full" / "Chr_1.breaks.tsv").read_text().splitlines()
    assert full[0].split("\t") == ["scaffold", "cut"] + ref.MOVES
    assert [ln.split("\t")[:2] for ln in full[1:]] == [["beta", "1"], ["beta", "2"], ["alpha", "3"], ["alpha", "2"], ["alpha", "1"]]
    assert [float(v) for v in full[3].split("\t")[2:]] == list(product[0]["table"][2])
    out = capsys.readouterr().out
    assert "Break support written for scaffolds 5" in out and "Broken group file written with scaffolds split 2" in out


def test_competing_mask_against_bin_orders_compared_as_lists():
    from hic_genome_assembler_amd import orderGenome as p2
    assert list(p2.BREAK_MOVES) == ref.MOVES
    for L in range(1, 9):
        before, after = [100, 101], [200]
        row0 = before + list(range(L)) + after
        whole_flip = before + list(range(L))[::-1] + after
        for min_piece in (1, 2, 3):
            mask = p2.break_counts(L, min_piece)
            assert mask.shape == (max(L - 1, 0), 8)
            for p in range(1, L):
                cand = [ref.candidate(row0, 2, L, p, k >> 2, (k >> 1) & 1, k & 1) for k in range(8)]
                assert cand[0] == row0 and cand[7] == whole_flip
                for k in range(8):
                    assert np.array_equal(p2._break_row(np.array(row0), 2, L, p, k), cand[k])
                    new = cand[k] != row0 and cand[k] != whole_flip and all(cand[k] != cand[e] for e in range(k))
                    assert bool(mask[p - 1, k]) == (new and min(p, L - p) >= min_piece), (L, p, k, min_piece)
    assert not p2.break_counts(2).any()                               # two bins: every candidate is A or its flip
    block = np.zeros((3, 8))
    block[0, 0] = 9.0                                                 # the arrangement itself never wins
    block[1, 3] = block[1, 4] = 5.0                                   # a tie: the first in enumeration order, both in the band
    block[2, 2] = 5.0 * (1 - 5e-10)                                   # ... and a third within 1e-9
    block[0, 2] = 8.0                                                 # reversing a one-bin piece does not count
    assert p2.break_summary(block, 4) == (11, 3)
    assert p2.break_summary(block, 4, 2) == (11, 2)                   # minPiece 2: only the middle cut
    assert p2.break_summary(block, 4, 3) == (-1, 0)


def test_command_line_and_config_handling(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run, supportBreaks as sb
    paths = gc.write_case_files("n160", str(tmp_path))
    cfg, files = _config(tmp_path, paths)
    v = run.readConfigFileToVariables(cfg)
    assert "breakSupportFile" not in v and "brokenChromosomeGroupFile" not in v and not run.ensureAllVariablesAreSet(v)
    args = sb._parse_args(["-config", cfg])
    assert (args.device, args.full, args.out, args.broken, args.minPiece, args.chromosomeOrderFile) == (0, None, None, None, 1, None)
    assert sb.resolve(args, v) == (files + "/chromosomeOrders.txt", os.path.join(files, "breakSupport.txt"), None)
    args = sb._parse_args(["-config", cfg, "-chromosomeOrderFile", "ref.txt", "-out", "o.txt", "-broken", "b.txt", "-minPiece", "3",
                           "-full", "d", "-device", "2"])
    assert sb.resolve(args, v) == ("ref.txt", "o.txt", "b.txt")
    assert (args.full, args.device, args.minPiece) == ("d", 2, 3)
    cfg2, files = _config(tmp_path, paths, breakSupportFile="breaks.txt", brokenChromosomeGroupFile="broken.txt")
    v2 = run.readConfigFileToVariables(cfg2)
    assert v2["breakSupportFile"] == files + "/breaks.txt" and v2["brokenChromosomeGroupFile"] == files + "/broken.txt"
    assert not run.ensureAllVariablesAreSet(v2)
    assert sb.resolve(sb._parse_args(["-config", cfg2]), v2)[1:] == (files + "/breaks.txt", files + "/broken.txt")
    assert {k: x for k, x in v2.items() if k not in ("breakSupportFile", "brokenChromosomeGroupFile")} == v
    with pytest.raises(SystemExit):
        sb._parse_args([])


def test_the_header_declares_the_two_exports(repo_root):
    with open(os.path.join(repo_root, "include", "hicmi.h")) as fh:
        header = fh.read()
    assert "int hicmi_p2_breaks(hicmi_ctx *ctx, const int32_t *ids, const uint8_t *rev, int64_t S, double total" in header
    assert "int hicmi_p2_breaks_multi(int64_t n_jobs, hicmi_ctx *const *ctxs" in header
    from hic_genome_assembler_amd import _lib
    assert {"hicmi_p2_breaks", "hicmi_p2_breaks_multi"} <= set(_lib.SIGNATURES)
