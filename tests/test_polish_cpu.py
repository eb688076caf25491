"""polishOrder without a GPU, on the NumPy stand-in context of tests/pairs_reference.py: single rounds against
the files supportEnds and placeUnplaced write, the mixed planted case to its fixed point, the flip rule on hand-built cases,
the stall, the round limit, the bytes of the order file and the refusals."""
import os

import numpy as np
import pytest

import anchor_reference as aref
import ends_reference as eref
import liftmap_reference as lref
import pairs_reference as ref
import test_anchor_cpu as anchor_cases
import test_ends_cpu as ends_cases

MIXED_FLIPS = [15, 18, 34]                       # planted flips of ends_reference that anchor_reference leaves in the order file


def _read(path):
    with open(path, newline="") as fh:
        return fh.read()


def _pairs(rows):
    sa, pa, sb, pb = zip(*rows)
    return (np.array(sa, np.int32), np.array(pa, np.int64), np.array(sb, np.int32), np.array(pb, np.int64))


def _polish(cfg, order, out, more=(), context=None):
    from hic_genome_assembler_amd import polishOrder
    context = ref.StandInContext() if context is None else context
    got = polishOrder.main(["-config", cfg, "-order", order, "-out", out] + list(more), context=context)
    assert context.calls[0] == "pairs_file" and context.calls.count("pairs_file") == 1      # one pass over the file
    assert context.calls[-1] == "pairs_drop" and context.store is None
    return got


def _summary(out):
    with open(os.path.join(out, "polish_summary.tsv")) as fh:
        head = dict(kv.split("=") for kv in fh.readline()[1:].rstrip("\n").split("\t"))
        rows = [line.rstrip("\n").split("\t") for line in fh if not line.startswith("#")]
    return head, rows


def _log(out):
    with open(os.path.join(out, "polish.log")) as fh:
        return [line.rstrip("\n").split("\t") for line in fh if not line.startswith("#")]


# ---- single rounds against the two tools ----------------------------------------------------------------------------------------
def test_one_place_round_writes_the_bytes_of_placeUnplaced_placed(tmp_path):
    from hic_genome_assembler_amd import placeUnplaced
    P = aref.planted()
    cfg, order, _save, _paths = anchor_cases._case_files(tmp_path, P["names"], P["sizes"], lref.order_file_text(P["chroms"], P["names"]),
                                                         P["pairs"])
    placed = str(tmp_path / "placed.txt")
    placeUnplaced.main(["-config", cfg, "-order", order, "-window", "5000", "-placed", placed], context=anchor_cases.StandInContext())
    out = str(tmp_path / "polished")
    status, rounds, log = _polish(cfg, order, out, ["-moves", "place", "-maxRounds", "1", "-window", "5000"])
    assert _read(os.path.join(out, "orders.txt")) == _read(placed) != _read(order)
    assert (status, rounds) == ("max_rounds", 1) and len(log) == 7 and {row[1] for row in log} == {"place"}     # scaf_30 is deferred
    # without the limit the deferred one follows in a second round, and a third finds nothing
    out2 = str(tmp_path / "polished2")
    status, rounds, log = _polish(cfg, order, out2, ["-moves", "place", "-window", "5000"])
    assert (status, rounds) == ("converged", 2) and [row[3] for row in log if row[0] == 2] == ["scaf_30"]
    assert _read(os.path.join(out2, "orders.txt")) == lref.order_file_text(P["true_chroms"], P["names"])


def test_the_first_flip_round_writes_the_bytes_of_supportEnds_flipped(tmp_path):
    from hic_genome_assembler_amd import supportEnds
    P = eref.planted()
    # the planted flips lie more than reach apart: one round takes them all
    where = {s: (q, k) for q, chrom in enumerate(P["chroms"]) for k, (s, _o) in enumerate(chrom)}
    for a in P["flips"]:
        for b in P["flips"]:
            assert a == b or where[a][0] != where[b][0] or abs(where[a][1] - where[b][1]) > eref.PLANTED_REACH
    cfg, order, _save, _paths = ends_cases._planted_files(tmp_path)
    flipped = str(tmp_path / "flipped.txt")
    supportEnds.main(["-config", cfg, "-order", order, "-window", "5000", "-flipped", flipped], context=ends_cases.FakeContext())
    out = str(tmp_path / "polished")
    status, rounds, log = _polish(cfg, order, out, ["-moves", "flip", "-maxRounds", "1", "-window", "5000"])
    assert _read(os.path.join(out, "orders.txt")) == _read(flipped) == lref.order_file_text(P["true_chroms"], P["names"])
    assert (status, rounds) == ("converged", 1)                                # nothing says flip after it: the limit was not in the way
    assert sorted(row[3] for row in log) == sorted(P["names"][s] for s in P["flips"]) and {row[0] for row in log} == {1}


# ---- the mixed planted case -----------------------------------------------------------------------------------------------------------
def mixed_files(tmp_path):
    """anchor_reference.planted() - eight scaffolds left out - with three of the scaffolds that stay given the wrong sign."""
    P = aref.planted()
    chroms = [[(s, ("+" if o == "-" else "-") if s in MIXED_FLIPS else o) for s, o in chrom] for chrom in P["chroms"]]
    assert all(any(s == f for chrom in chroms for s, _o in chrom) for f in MIXED_FLIPS)
    cfg, order, save, _paths = anchor_cases._case_files(tmp_path, P["names"], P["sizes"], lref.order_file_text(chroms, P["names"]), P["pairs"])
    return cfg, order, save


def check_mixed_outputs(polished):
    """The polished order file of the mixed case is the true layout (also used by the GPU round trip)."""
    P = aref.planted()
    assert polished == lref.order_file_text(P["true_chroms"], P["names"])


def test_the_mixed_planted_case_converges_to_the_true_layout(tmp_path, capsys):
    from hic_genome_assembler_amd import placeUnplaced, supportEnds
    cfg, order, save = mixed_files(tmp_path)
    before = _read(order)
    out = str(tmp_path / "polished")
    status, rounds, log = _polish(cfg, order, out, ["-window", "5000"])
    assert status == "converged" and _read(order) == before                     # the input order file is never changed
    polished = os.path.join(out, "orders.txt")
    check_mixed_outputs(_read(polished))
    P = aref.planted()
    assert sorted(row[3] for row in log if row[1] == "flip") == sorted(P["names"][s] for s in MIXED_FLIPS)
    assert sorted(row[3] for row in log if row[1] == "place") == sorted(P["names"][s] for s in P["removed"])
    assert [int(row[0]) for row in log] == sorted(int(row[0]) for row in log) and int(log[-1][0]) == rounds
    head, rows = _summary(out)
    assert head["status"] == "converged" and int(head["rounds"]) == rounds and head["moves"] == "flip,place"
    assert head["ended"] == "nothing_left"
    n = len(P["pairs"][0])
    assert (int(head["lines"]), int(head["used"])) == (n, n) and int(head["pairs_kept"]) + int(head["pairs_intra"]) == n
    assert int(head["pairs_kept"]) == int(ref.mask(P["pairs"]).sum())
    assert [int(r[1]) for r in rows] == [len(c) for c in P["chroms"]] and [int(r[2]) for r in rows] == [len(c) for c in P["true_chroms"]]
    assert sum(int(r[3]) for r in rows) == 3 and sum(int(r[4]) for r in rows) == 8 and all(int(r[6]) > int(r[5]) for r in rows)
    assert "POLISH: converged after %d round(s): 3 flip(s), 8 insertion(s)" % rounds in capsys.readouterr().out
    # on that output the two tools have nothing left to do
    report = str(tmp_path / "ends.txt")
    supportEnds.main(["-config", cfg, "-order", polished, "-window", "5000", "-out", report], context=ends_cases.FakeContext())
    assert "\tflip\n" not in _read(report) and _read(report).count("\tsupported\n") == 40
    report = str(tmp_path / "unplaced.txt")
    placeUnplaced.main(["-config", cfg, "-order", polished, "-window", "5000", "-out", report], context=anchor_cases.StandInContext())
    assert not any(word in _read(report) for word in ("\tplaced\n", "\torientation_open\n", "\tdeferred\n"))
    assert os.listdir(save) == [] or set(os.listdir(save)) <= {"endSupport.txt", "unplacedSupport.txt"}


def test_the_round_limit_says_max_rounds(tmp_path):
    cfg, order, _save = mixed_files(tmp_path)
    out = str(tmp_path / "polished")
    status, rounds, log = _polish(cfg, order, out, ["-window", "5000", "-maxRounds", "1"])
    assert (status, rounds) == ("max_rounds", 1) and {row[0] for row in log} == {1} and {row[1] for row in log} == {"flip"}
    assert _summary(out)[0]["status"] == "max_rounds" and _summary(out)[0]["ended"] == "round_limit"
    P = aref.planted()
    chroms = [[(s, o) for s, o in chrom if s not in P["removed"]] for chrom in P["true_chroms"]]
    assert _read(os.path.join(out, "orders.txt")) == lref.order_file_text(chroms, P["names"])      # the flips are made, nothing is placed


# ---- the flip rule on hand-built cases ------------------------------------------------------------------------------------------------
H_NAMES = ["a", "b", "c", "d", "e", "f", "g", "h"]
H_SIZES = np.full(8, 10, dtype=np.int64)
A, B, C, D, E, F, G, H = range(8)
H_ORDER = ("### Chromosome grouping 1 ###\r\na\t+\r\nb\t+\tnote\r\nc\t+\r\nd\t+\n### Chromosome grouping 2 ###\ne\t+\nf\t+\ng\t+\nh\t+")
# window 2: the bases 1, 2 of a + scaffold are its left zone, 9, 10 its right zone.
# Chr_1: b and c both say flip (5 and 4 against the one link they have as they lie), and flipping both would leave none.
# Chr_2: f and g are both the wrong way round: each says flip from its outer neighbour, and once f is turned g has 14 reasons.
H_ROWS = [(B, 1, C, 1)] * 5 + [(B, 10, C, 10)] * 4 + [(B, 10, C, 1)] + [(E, 10, F, 10)] * 6 + [(G, 1, H, 1)] * 6 + [(F, 1, G, 10)] * 8 \
    + [(A, 5, A, 6)] * 3 + [(A, 1, E, 1)]


def _facing(chroms, sizes, pairs, window, reach):
    tables = lref.layout(chroms, sizes, 100, drop_unplaced=True)
    return int(eref.table(pairs, sizes, tables, window, reach)[0][:, :, eref.RL].sum())


def test_two_flips_within_reach_take_turns_and_facing_links_rise_every_round(tmp_path):
    pairs = _pairs(H_ROWS)
    cfg, order, _save, _paths = anchor_cases._case_files(tmp_path, H_NAMES, H_SIZES, H_ORDER, pairs)
    chroms = [[(s, "+") for s in (A, B, C, D)], [(s, "+") for s in (E, F, G, H)]]

    def lying(flipped):
        return [[(s, "-" if s in flipped else "+") for s, _o in chrom] for chrom in chroms]

    assert _facing(lying({B, C}), H_SIZES, pairs, 2, 1) < _facing(chroms, H_SIZES, pairs, 2, 1) == 1       # both at once lower F
    out = str(tmp_path / "polished")
    status, rounds, log = _polish(cfg, order, out, ["-moves", "flip", "-window", "2", "-reach", "1", "-minPairs", "4"])
    assert (status, rounds) == ("converged", 2)
    assert [row[:6] for row in _log(out)] == [["1", "flip", "2", "f", "0", "6"], ["1", "flip", "1", "b", "1", "5"],
                                              ["2", "flip", "2", "g", "0", "14"]]
    seen, flipped = [_facing(chroms, H_SIZES, pairs, 2, 1)], set()
    for r in (1, 2):
        flipped |= {H_NAMES.index(row[3]) for row in log if row[0] == r}
        seen.append(_facing(lying(flipped), H_SIZES, pairs, 2, 1))
    assert seen == [1, 11, 25]
    # line endings, the third column and the missing final newline are kept
    assert _read(os.path.join(out, "orders.txt")) == H_ORDER.replace("b\t+\tnote", "b\t-\tnote").replace("f\t+\n", "f\t-\n").replace("g\t+\n", "g\t-\n")
    head, rows = _summary(out)
    assert [r[3] for r in rows] == ["1", "2"] and [r[5:] for r in rows] == [["1", "5"], ["0", "20"]] and head["pairs_intra"] == "3"


def test_a_round_that_does_not_raise_the_facing_links_is_undone_and_says_stalled(tmp_path):
    # b has three bases at a window of 5: its middle base is in its left zone whichever way round it lies
    names, sizes = ["a", "b", "c"], np.array([10, 3, 10], dtype=np.int64)
    text = "### Chromosome grouping 1 ###\na\t+\nb\t+\nc\t+\n"
    pairs = _pairs([(1, 2, 2, 1)] * 5)
    cfg, order, _save, _paths = anchor_cases._case_files(tmp_path, names, sizes, text, pairs)
    out = str(tmp_path / "polished")
    ctx = ref.StandInContext()
    status, rounds, log = _polish(cfg, order, out, ["-window", "5", "-reach", "1"], context=ctx)
    assert (status, rounds, log) == ("stalled", 0, []) and _read(os.path.join(out, "orders.txt")) == text
    assert ctx.calls.count("ends_resident") == 2 and _summary(out)[0]["status"] == "stalled" and _log(out) == []
    assert _summary(out)[0]["ended"] == "nothing_left"


def test_a_stalled_run_still_places_and_says_how_the_loop_ended(tmp_path):
    # the stall above, and d left out of the order file: six links of its first half with c's right end put it behind c
    names, sizes = ["a", "b", "c", "d"], np.array([10, 3, 10, 10], dtype=np.int64)
    text = "### Chromosome grouping 1 ###\na\t+\nb\t+\nc\t+\n"
    pairs = _pairs([(1, 2, 2, 1)] * 5 + [(3, 1, 2, 10)] * 6)
    cfg, order, _save, _paths = anchor_cases._case_files(tmp_path, names, sizes, text, pairs)
    out = str(tmp_path / "polished")
    status, rounds, log = _polish(cfg, order, out, ["-window", "5", "-reach", "1"])
    assert (status, rounds) == ("stalled", 1) and [row[:7] for row in log] == [(1, "place", 1, "d", "c", "end", "+")]
    assert _read(os.path.join(out, "orders.txt")) == text + "d\t+\n"
    head, rows = _summary(out)
    assert (head["status"], head["ended"]) == ("stalled", "nothing_left") and rows[0][1:5] == ["3", "4", "0", "1"]
    # the same under a limit of one round: the place round is applied, and nothing is left after it
    out = str(tmp_path / "limited")
    assert _polish(cfg, order, out, ["-window", "5", "-reach", "1", "-maxRounds", "1"])[:2] == ("stalled", 1)
    assert _summary(out)[0]["ended"] == "nothing_left"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import polishOrder, synth
    cfg, order, save = mixed_files(tmp_path)
    d = str(tmp_path)
    out = os.path.join(d, "polished")
    ctx = ref.StandInContext()

    def write(text, name):
        path = os.path.join(d, name)
        with open(path, "w") as fh:
            fh.write(text)
        return path

    def refused(word, more=(), config=cfg, order_file=order, out_dir=out):
        args = ["-config", config, "-out", out_dir] + (["-order", order_file] if order_file else [])
        with pytest.raises(SystemExit) as exc:
            polishOrder.main(args + list(more), context=ctx)
        assert word in str(exc.value.code) and str(exc.value.code).startswith("ERROR... ") and \
            str(exc.value.code).endswith(" Exiting..."), exc.value.code

    refused("moves", ["-moves", "flip,swap"])
    refused("moves", ["-moves", ""])
    refused("moves", ["-moves", "place,"])
    refused("maxRounds", ["-maxRounds", "0"])
    refused("maxRounds", ["-maxRounds", "-3"])
    refused("window", ["-window", "0"])
    refused("reach", ["-reach", "0"])
    refused("reach", ["-reach", "65"])
    refused("minPairs", ["-minPairs", "-1"])
    refused("minSize", ["-minSize", "-1"])
    refused("minRatio", ["-minRatio", "0.5"])
    refused("zz", order_file=write("### 1 ###\nscaf_2\t+\nzz\t+\n", "unknown.txt"))
    refused("twice", order_file=write("### 1 ###\nscaf_2\t+\n### 2 ###\nscaf_5\t+\nscaf_2\t-\n", "twice.txt"))
    refused("orientation", order_file=write("### 1 ###\nscaf_2\t+\nscaf_5\t?\n", "orient.txt"))
    refused("does not exist", order_file=os.path.join(d, "nothing_here"))
    refused("does not exist", order_file=None)                               # neither default order file is there
    refused("replace", out_dir=os.path.dirname(order))                       # the polished file would be the input
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    refused("validPairFile", config=synth.write_config(os.path.join(d, "c2.txt"), paths, save, os.path.join(d, "plots"), 100000))
    # 2^19 + 1 scaffolds at reach 64, one of them placed: placing the others would pass the table
    n = 2 ** 19 + 1
    big = dict(paths, hicProScaffSizeFile=write("".join("s%d\t1\n" % k for k in range(n)), "big.sizes"))
    big_cfg = synth.write_config(os.path.join(d, "big.txt"), big, save, os.path.join(d, "plots"), 100000,
                                 extra={"validPairFile": os.path.join(d, "case.allValidPairs")})
    refused("%d counters" % (n * 256), ["-reach", "64"], config=big_cfg, order_file=write("### 1 ###\ns0\t+\n", "big.order"))
    assert ctx.calls == [] and not os.path.exists(out) and os.listdir(save) == []
