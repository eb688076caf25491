"""The command lines of the six pair tools - supportSpans, supportEnds, placeUnplaced, supportSeats, polishOrder and
scaffoldLinks - as a table of invocations on the stand-in contexts of the CPU tests, and ``run_case``, which runs one and
returns what can be seen of it from outside: what it printed, how it exited, a digest of what it returned, every file it
wrote and the calls it made on its context.  ``python tests/pairtool_cases.py --record`` writes that for every case to
tests/records/pairtools.json; tests/test_pairtool_cpu.py holds the tools to the record."""
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "records", "pairtools.json")
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import anchor_reference as aref                                              # noqa: E402
import buildmap_reference as bref                                            # noqa: E402
import ends_reference as eref                                                # noqa: E402
import links_lifted_reference as lifted_ref                                  # noqa: E402
import links_reference as links_ref                                          # noqa: E402
import pairs_reference as pref                                               # noqa: E402
import test_anchor_cpu as anchor_cases                                       # noqa: E402
import test_ends_cpu as ends_cases                                           # noqa: E402
import test_links_cpu as links_cases                                         # noqa: E402
import test_polish_cpu as polish_cases                                       # noqa: E402
import test_seats_cpu as seats_cases                                         # noqa: E402
import test_spans_cpu as spans_cases                                         # noqa: E402

HICPRO_KEYS = ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")


# ---- the stand-ins -------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Passes everything on to a stand-in context and notes the name of every method the tool calls on it, in order.  An
    attribute the stand-in does not have is missing here too, so ``hasattr`` answers as it does on the stand-in."""

    def __init__(self, inner):
        self._inner, self.called = inner, []

    def __getattr__(self, name):
        attr = getattr(self._inner, name)
        if not callable(attr):
            return attr

        def call(*args, **kwargs):
            self.called.append(name)
            return attr(*args, **kwargs)
        return call


class AnchorFileContext:
    """``anchor_file`` of _lib, answered by the reference on the file's pairs: a context that answers a pass in one call."""

    def anchor_file(self, path, names, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window, threads=0):
        with open(path, "rb") as fh:
            got, stats, _after = bref.parse_text(fh.read(), names, sizes)
        tables = (np.asarray(lift_seq, np.int32), np.asarray(lift_off, np.int64), np.asarray(lift_rev, np.uint8), np.asarray(seq_sizes, np.int64))
        return (stats + (1,), aref.number_blocks(sizes, tables, target)[0]) + aref.table(got, sizes, tables, target, window)


WIDE_S, WIDE_N = 2 ** 12, 2 ** 12 + 2 ** 13 + 1


class WideCountsOnly:
    """Pass 1 of the wide case - every unplaced scaffold one link with the one chromosome - without the reference's loops."""

    def anchor_file(self, path, names, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window, threads=0):
        assert target is None
        n, S = WIDE_N, WIDE_S
        first = np.where(np.arange(n) >= S, np.arange(n) - S, -1).astype(np.int64)
        return (n - S, n - S, 0, 0, 1), first, np.ones(n - S, np.uint64), np.array([n - S, 0, 0, 0, 0, 0], np.uint64)


class RefusingLinks(links_ref.StandInContext):
    def links_resident(self, sizes, window):
        from hic_genome_assembler_amd import _lib
        raise _lib.HicmiError("libhicmi error -5: the link table needs 4294967296 slots")


class RefusingLifted(lifted_ref.StandInContext):
    def links_lifted(self, *args):
        from hic_genome_assembler_amd import _lib
        raise _lib.HicmiError("libhicmi error -1: the tables are refused")


CONTEXTS = {"spans": spans_cases.FakeContext, "ends": ends_cases.FakeContext, "anchor": anchor_cases.StandInContext,
            "anchor_file": AnchorFileContext, "wide_counts": WideCountsOnly, "seats": seats_cases.StandInContext,
            "pairs": pref.StandInContext, "links": links_ref.StandInContext, "lifted": lifted_ref.StandInContext,
            "refusing_links": RefusingLinks, "refusing_lifted": RefusingLifted}


# ---- the inputs: each returns the words a case's arguments may name as {word} -------------------------------------------------------
def _named(cfg, order, save, paths):
    return {"cfg": cfg, "order": order, "save": save, "_paths": paths}


def _paths_in(d):
    return {k: os.path.join(d, k + ".txt") for k in HICPRO_KEYS}


def spans_planted(d):
    return _named(*spans_cases._planted_files(d))


def ends_planted(d):
    return _named(*ends_cases._planted_files(d))


def six(d):
    """The six-scaffold assembly of test_ends_cpu: an empty scaffold, an unplaced one, a chromosome of one scaffold, CR LF
    lines, a third column and no final newline."""
    A, B, C, D, E = ends_cases.A, ends_cases.B, ends_cases.C, ends_cases.D, ends_cases.E
    rows = [(C, 7, B, 1)] * 3 + [(A, 1, C, 7)] * 2 + [(C, 1, B, 1)] + [(A, 5, B, 1)] * 2 + [(A, 1, B, 1)] * 2 \
        + [(E, 1, A, 1), (D, 1, A, 1), (C, 4, A, 1), (C, 2, C, 3)]
    text = "### Chromosome grouping 1 ###\r\nc\t-\tnote\r\nb\t-\r\na\t+\n### Chromosome grouping 2 ###\nd\t+\nf\t+"
    return _named(*anchor_cases._case_files(d, ends_cases.NAMES, ends_cases.SIZES, text, ends_cases._pairs(rows)))


def anchor_verdicts(d):
    return _named(*anchor_cases._case_files(d, anchor_cases.V_NAMES, anchor_cases.V_SIZES, anchor_cases.V_ORDER, anchor_cases._verdict_pairs()))


def anchor_nothing(d):
    return _named(*anchor_cases._case_files(d, ["a", "b", "c"], np.array([10, 0, 10]), "### 1 ###\na\t+\nc\t-\n", anchor_cases._pairs([(0, 1, 2, 1)])))


def seats_displaced(d):
    return _named(*(seats_cases.displaced_files(d) + (_paths_in(d),)))


def seats_verdicts(d):
    return _named(*anchor_cases._case_files(d, seats_cases.V_NAMES, seats_cases.V_SIZES, seats_cases.V_ORDER,
                                            seats_cases._pairs(seats_cases._verdict_rows())))


def polish_mixed(d):
    return _named(*(polish_cases.mixed_files(d) + (_paths_in(d),)))


def polish_hand(d):
    return _named(*anchor_cases._case_files(d, polish_cases.H_NAMES, polish_cases.H_SIZES, polish_cases.H_ORDER, polish_cases._pairs(polish_cases.H_ROWS)))


def links_verdicts(d):
    text = "### Chromosome grouping 1 ###\nA\t+\nB\t+\nC\t+\n### Chromosome grouping 2 ###\nF\t-\nD\t-\n"
    return _named(*anchor_cases._case_files(d, links_cases.V_NAMES, links_cases.V_SIZES, text, links_cases._pairs(links_cases.V_ROWS)))


def links_empty(d):
    return _named(*anchor_cases._case_files(d, links_cases.V_NAMES, links_cases.V_SIZES, "", links_cases._pairs([(links_cases.C, 4, links_cases.C, 5)] * 3)))


def links_planted(d):
    _P, cfg, order, save = links_cases.planted_files(d)
    return _named(cfg, order, save, _paths_in(d))


def _write(d, name, text):
    path = os.path.join(d, name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def _config(d, name, paths, save, pair_file=None):
    from hic_genome_assembler_amd import synth
    extra = None if pair_file is None else {"validPairFile": pair_file}
    return synth.write_config(os.path.join(d, name), paths, save, os.path.join(d, "plots"), 100000, extra=extra)


def _pair_file(d):
    return os.path.join(d, "planted.allValidPairs" if os.path.exists(os.path.join(d, "planted.allValidPairs")) else "case.allValidPairs")


def more_configs(d, w):
    """{no_pairs}: a config without validPairFile; {missing_pairs}: one that names a file that is not there."""
    w["no_pairs"] = _config(d, "c2.txt", w["_paths"], w["save"])
    w["missing_pairs"] = _config(d, "c3.txt", w["_paths"], w["save"], os.path.join(d, "no_such_pairs"))


def _big(d, w, names, order_text, pair_file=None):
    big = dict(w["_paths"], hicProScaffSizeFile=_write(d, "big.sizes", "".join("%s\t1\n" % x for x in names)))
    w["big_cfg"] = _config(d, "big.txt", big, w["save"], pair_file or _pair_file(d))
    w["big_order"] = _write(d, "big.order", order_text)


def big_cells(d, w):
    """2^27 + 1 cells at step 1."""
    big = dict(w["_paths"], hicProScaffSizeFile=_write(d, "big.sizes", "scaf_1\t%d\nscaf_2\t1\n" % 2 ** 27))
    w["big_cfg"] = _config(d, "big.txt", big, w["save"], _pair_file(d))


def big_reach(d, w):
    """2^19 + 1 placed scaffolds: at reach 64 one entry past the table."""
    n = 2 ** 19 + 1
    _big(d, w, ["s%d" % k for k in range(n)], "### 1 ###\n" + "".join("s%d\t+\n" % k for k in range(n)))


def big_reach_one_placed(d, w):
    """2^19 + 1 scaffolds, one of them placed: placing the others would pass the table at reach 64."""
    _big(d, w, ["s%d" % k for k in range(2 ** 19 + 1)], "### 1 ###\ns0\t+\n")


def big_pass1(d, w):
    """2^14 + 1 unplaced scaffolds against 2^13 chromosomes: one block past the table."""
    n_seq = 2 ** 13
    _big(d, w, ["s%d" % k for k in range(n_seq + 2 ** 14 + 1)], "".join("### %d ###\ns%d\t+\n" % (k, k) for k in range(n_seq)))


def big_pass2(d, w):
    """2^13 + 1 scaffolds that get the one chromosome of 2^12 scaffolds: 4 x 2^12 counters each."""
    names = ["s%d" % k for k in range(WIDE_N)]
    pairs = _write(d, "wide.pairs", "".join("r\t%s\t1\t+\ts0\t1\t-\n" % names[k] for k in range(WIDE_S, WIDE_N)))
    _big(d, w, names, "### 1 ###\n" + "".join("%s\t+\n" % x for x in names[:WIDE_S]), pairs)


def big_seats(d, w):
    """5,793 scaffolds in one chromosome: 5793 x (1 + 4 x 5793) counters pass 2^27."""
    n = 5793
    _big(d, w, ["s%d" % k for k in range(n)], "### 1 ###\n" + "".join("s%d\t+\n" % k for k in range(n)))


SETUPS = {f.__name__: f for f in (spans_planted, ends_planted, six, anchor_verdicts, anchor_nothing, seats_displaced, seats_verdicts,
                                  polish_mixed, polish_hand, links_verdicts, links_empty, links_planted)}
EXTRAS = {f.__name__: f for f in (more_configs, big_cells, big_reach, big_reach_one_placed, big_pass1, big_pass2, big_seats)}


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def case(cid, tool, setup, args, context, extras=(), files=None):
    """``args``: the command line, split at blanks; {word} names a path of the setup, {d} the directory of the case.
    ``files``: {name: text} written into {d} before the run."""
    return {"id": cid, "tool": tool, "setup": setup, "args": args.split(" ") if isinstance(args, str) else list(args), "context": context,
            "extras": tuple(extras), "files": files or {}}


def bad_order_files(n1, n2):
    return {"unknown.txt": "### 1 ###\n%s\t+\nzz\t+\n" % n1, "twice.txt": "### 1 ###\n%s\t+\n### 2 ###\n%s\t+\n%s\t-\n" % (n1, n2, n1),
            "orient.txt": "### 1 ###\n%s\t+\n%s\t?\n" % (n1, n2), "empty.txt": "### 1 ###\n%s\t+\n### 2 ###\n" % n1,
            "one_column.txt": "### 1 ###\n%s\n" % n1}


def refusals(tool, setup, context, base, rows, names, with_order=True):
    """One case per row (word, more arguments, extras).  ``more`` may name -config or -order itself; else the setup's config
    is given, and with ``with_order`` its order file unless ``more`` starts with !order."""
    out = []
    for word, more, extras in rows:
        more = more.split(" ") if isinstance(more, str) else list(more)
        no_order = more[:1] == ["!order"] or "-order" in more or "-scaffolds" in more or not with_order
        more = more[1:] if more[:1] == ["!order"] else more
        args = base.split(" ") + ([] if "-config" in more else ["-config", "{cfg}"]) + ([] if no_order else ["-order", "{order}"])
        out.append(case("%s-refused-%s" % (tool, word), tool, setup, args + more, context, extras, bad_order_files(*names)))
    return out


ORDER_ROWS = [(w, "-order {d}/%s.txt" % w, ()) for w in ("unknown", "twice", "orient", "empty", "one_column")] + \
    [("missing_order", "-order {d}/nothing_here", ()), ("no_default_order", "!order", ())]
NO_PAIRS = [("no_pairs", "-config {no_pairs}", ("more_configs",)),
            ("two_no_pairs_missing_order", "-config {no_pairs} -order {d}/nothing_here", ("more_configs",))]
MISSING_PAIRS = [("missing_pairs", "-config {missing_pairs}", ("more_configs",))]

CASES = []

# supportSpans
CASES += [
    case("spans-all", "supportSpans", "spans_planted", "-config {cfg} -order {order} -step 1000 -cuts {d}/cuts.tsv -full {d}/full -threads 2", "spans"),
    case("spans-scaffolds", "supportSpans", "spans_planted",
         "-config {cfg} -scaffolds -step 1000 -flank 5 -out {d}/own.txt -cuts {d}/cuts.tsv -full {d}/full", "spans"),
    case("spans-six", "supportSpans", "six", "-config {cfg} -order {order} -step 2 -flank 1 -minRatio 0.5 -out {d}/r.txt -cuts {d}/cuts.tsv -full {d}/full",
         "spans"),
    case("spans-six-gap0", "supportSpans", "six", "-config {cfg} -order {order} -step 1 -flank 2 -gap 0 -maxSpan 6 -out {d}/r.txt", "spans"),
    case("spans-help", "supportSpans", "spans_planted", "--help", "spans"),
]
CASES += refusals("supportSpans", "spans_planted", "spans", "-out {d}/report.txt -cuts {d}/report.txt.cuts -full {d}/report.txt.full", [
    ("step_0", "-step 0", ()), ("step_neg", "-step -5", ()), ("flank_0", "-flank 0", ()), ("flank_4097", "-flank 4097", ()),
    ("maxSpan", "-maxSpan -1", ()), ("gap", "-gap -1", ()), ("scaffolds_with_order", "-order {order} -scaffolds", ())] + ORDER_ROWS + [
    ("big", "-config {big_cfg} -step 1 -scaffolds", ("big_cells",))] + NO_PAIRS + [
    ("two_step_flank", "-step 0 -flank 0", ()), ("two_flank_maxSpan", "-flank 0 -maxSpan -1", ()), ("two_maxSpan_gap", "-maxSpan -1 -gap -1", ()),
    ("two_gap_no_pairs", "-gap -1 -config {no_pairs}", ("more_configs",))], ("scaf_1", "scaf_2"))

# supportEnds
CASES += [
    case("ends-all", "supportEnds", "ends_planted", "-config {cfg} -order {order} -window 5000 -flipped {d}/flipped.txt -full {d}/full -threads 2", "ends"),
    case("ends-six", "supportEnds", "six",
         "-config {cfg} -order {order} -window 1 -reach 2 -minPairs 2 -out {d}/r.txt -flipped {d}/flipped.txt -full {d}/full", "ends"),
    case("ends-help", "supportEnds", "ends_planted", "--help", "ends"),
]
CASES += refusals("supportEnds", "ends_planted", "ends", "-out {d}/report.txt -flipped {d}/report.txt.flipped -full {d}/report.txt.full", [
    ("window_0", "-window 0", ()), ("window_neg", "-window -5", ()), ("reach_0", "-reach 0", ()), ("reach_65", "-reach 65", ()),
    ("minPairs", "-minPairs -1", ())] + ORDER_ROWS + [
    ("big", "-config {big_cfg} -order {big_order} -reach 64", ("big_reach",))] + NO_PAIRS + MISSING_PAIRS + [
    ("two_window_reach", "-window 0 -reach 0", ()), ("two_reach_minPairs", "-reach 65 -minPairs -1", ()),
    ("two_minPairs_no_pairs", "-minPairs -1 -config {no_pairs}", ("more_configs",))], ("scaf_1", "scaf_2"))

# placeUnplaced
CASES += [
    case("place-all", "placeUnplaced", "anchor_verdicts",
         "-config {cfg} -order {order} -window 10 -reach 1 -minSize 10 -placed {d}/placed.txt -full {d}/full -threads 2", "anchor"),
    case("place-anchor-file", "placeUnplaced", "anchor_verdicts", "-config {cfg} -order {order} -window 10 -reach 2 -out {d}/report.txt -placed {d}/placed.txt",
         "anchor_file"),
    case("place-reach-64", "placeUnplaced", "anchor_verdicts", "-config {cfg} -order {order} -window 10 -reach 64 -out {d}/report.txt", "anchor"),
    case("place-six", "placeUnplaced", "six",
         "-config {cfg} -order {order} -window 1 -reach 2 -minPairs 1 -minRatio 1 -out {d}/r.txt -placed {d}/placed.txt -full {d}/full", "anchor"),
    case("place-nothing-unplaced", "placeUnplaced", "anchor_nothing", "-config {cfg} -order {order} -placed {d}/placed.txt", "anchor"),
    case("place-help", "placeUnplaced", "anchor_verdicts", "--help", "anchor"),
]
CASES += refusals("placeUnplaced", "anchor_verdicts", "anchor", "-out {d}/report.txt -placed {d}/report.txt.placed -full {d}/report.txt.full", [
    ("window_0", "-window 0", ()), ("window_neg", "-window -5", ()), ("reach_0", "-reach 0", ()), ("reach_65", "-reach 65", ()),
    ("minPairs", "-minPairs -1", ()), ("minSize", "-minSize -1", ()), ("minRatio", "-minRatio 0.99", ()), ("minRatio_nan", "-minRatio nan", ())]
    + ORDER_ROWS + [("big_pass1", "-config {big_cfg} -order {big_order}", ("big_pass1",))] + NO_PAIRS + MISSING_PAIRS + [
    ("two_window_minSize", "-window 0 -minSize -1", ()), ("two_reach_minPairs", "-reach 0 -minPairs -1", ()),
    ("two_minPairs_minSize", "-minPairs -1 -minSize -1", ()), ("two_minSize_minRatio", "-minSize -1 -minRatio 0.5", ()),
    ("two_minRatio_no_pairs", "-minRatio 0.5 -config {no_pairs}", ("more_configs",))], ("p1", "p2"))
CASES += refusals("placeUnplaced", "anchor_verdicts", "wide_counts", "-out {d}/report.txt -placed {d}/report.txt.placed -full {d}/report.txt.full", [
    ("big_pass2", "-config {big_cfg} -order {big_order} -minPairs 1", ("big_pass2",))], ("p1", "p2"))

# supportSeats
CASES += [
    case("seats-all", "supportSeats", "seats_displaced", "-config {cfg} -order {order} -window 5000 -moved {d}/moved.txt -out {d}/seats.txt -full {d}/full",
         "seats"),
    case("seats-verdicts", "supportSeats", "seats_verdicts", "-config {cfg} -order {order} -window 5 -reach 1 -moved {d}/moved.txt -full {d}/full -threads 2",
         "seats"),
    case("seats-six", "supportSeats", "six",
         "-config {cfg} -order {order} -window 1 -reach 2 -minPairs 1 -minRatio 1 -out {d}/r.txt -moved {d}/moved.txt -full {d}/full", "seats"),
    case("seats-help", "supportSeats", "seats_displaced", "--help", "seats"),
]
CASES += refusals("supportSeats", "seats_displaced", "seats", "-out {d}/seats.txt", [
    ("window_0", "-window 0", ()), ("reach_0", "-reach 0", ()), ("reach_65", "-reach 65", ()), ("minPairs", "-minPairs -1", ()),
    ("minRatio", "-minRatio 0.5", ())] + [r for r in ORDER_ROWS if r[0] not in ("empty", "one_column")] + NO_PAIRS + [
    ("big", "-config {big_cfg} -order {big_order}", ("big_seats",)),
    ("two_window_reach", "-window 0 -reach 65", ()), ("two_reach_minRatio", "-reach 0 -minRatio 0.5", ()),
    ("two_minPairs_minRatio", "-minPairs -1 -minRatio 0.5", ()), ("two_minRatio_no_pairs", "-minRatio 0.5 -config {no_pairs}", ("more_configs",))],
    ("scaf_2", "scaf_5"))

# polishOrder
CASES += [
    case("polish-all", "polishOrder", "polish_mixed", "-config {cfg} -order {order} -out {d}/polished -moves flip,place,relocate -window 5000 -threads 2",
         "seats"),
    case("polish-default-moves", "polishOrder", "polish_mixed", "-config {cfg} -order {order} -out {d}/polished -window 5000", "pairs"),
    case("polish-max-rounds", "polishOrder", "polish_mixed", "-config {cfg} -order {order} -out {d}/polished -window 5000 -maxRounds 1", "pairs"),
    case("polish-relocate", "polishOrder", "seats_displaced", "-config {cfg} -order {order} -out {d}/polished -moves flip,relocate -window 5000", "seats"),
    case("polish-hand-flips", "polishOrder", "polish_hand", "-config {cfg} -order {order} -out {d}/polished -moves flip -window 2 -reach 1 -minPairs 4", "pairs"),
    case("polish-six", "polishOrder", "six",
         "-config {cfg} -order {order} -out {d}/polished -moves flip,place,relocate -window 1 -reach 2 -minPairs 1 -minRatio 1", "seats"),
    case("polish-help", "polishOrder", "polish_mixed", "--help", "pairs"),
]
CASES += refusals("polishOrder", "polish_mixed", "pairs", "-out {d}/polished", [
    ("moves_swap", ["-moves", "flip,swap"], ()), ("moves_empty", ["-moves", ""], ()), ("moves_place_comma", ["-moves", "place,"], ()),
    ("moves_relocate_comma", ["-moves", "relocate,"], ()), ("maxRounds_0", "-maxRounds 0", ()), ("maxRounds_neg", "-maxRounds -3", ()),
    ("window_0", "-window 0", ()), ("reach_0", "-reach 0", ()), ("reach_65", "-reach 65", ()), ("minPairs", "-minPairs -1", ()),
    ("minSize", "-minSize -1", ()), ("minRatio", "-minRatio 0.5", ())] + [r for r in ORDER_ROWS if r[0] not in ("empty", "one_column")] + [
    ("replace", "-out {d}", ())] + NO_PAIRS + [
    ("big", "-config {big_cfg} -order {big_order} -reach 64", ("big_reach_one_placed",)),
    ("big_relocate", "-config {big_cfg} -order {big_order} -moves flip,relocate", ("big_seats",)),
    ("two_moves_maxRounds", "-moves flip,swap -maxRounds 0", ()), ("two_maxRounds_window", "-maxRounds 0 -window 0", ()),
    ("two_window_reach", "-window 0 -reach 0", ()), ("two_minPairs_minSize", "-minPairs -1 -minSize -1", ()),
    ("two_minSize_minRatio", "-minSize -1 -minRatio 0.5", ()), ("two_minRatio_no_pairs", "-minRatio 0.5 -config {no_pairs}", ("more_configs",)),
    ("two_missing_order_replace", "-order {d}/nothing_here -out {d}", ())], ("scaf_2", "scaf_5"))

# scaffoldLinks
CASES += [
    case("links-all", "scaffoldLinks", "links_planted", "-config {cfg} -out {d}/links -window 5000 -rounds 3 -order {order} -threads 2", "lifted"),
    case("links-growth", "scaffoldLinks", "links_planted", "-config {cfg} -out {d}/links -window 5000 -rounds 5 -growth 2 -gap 0", "lifted"),
    case("links-verdicts", "scaffoldLinks", "links_verdicts", "-config {cfg} -out {d}/links -window 2 -minSize 5 -order {order}", "links"),
    case("links-empty", "scaffoldLinks", "links_empty", "-config {cfg} -out {d}/out -window 2", "links"),
    case("links-six", "scaffoldLinks", "six", "-config {cfg} -out {d}/links -window 1 -minPairs 2 -minRatio 1 -rounds 3 -order {order}", "lifted"),
    case("links-help", "scaffoldLinks", "links_verdicts", "--help", "links"),
]
CASES += refusals("scaffoldLinks", "links_verdicts", "links", "-out {d}/links", [
    ("window_0", "-window 0", ()), ("minPairs", "-minPairs -1", ()), ("minSize", "-minSize -1", ()), ("minRatio", "-minRatio 0.99", ())]
    + NO_PAIRS + MISSING_PAIRS + [r for r in ORDER_ROWS if r[0] in ("unknown", "twice", "orient", "missing_order")] + [
    ("rounds_0", "-rounds 0", ()), ("rounds_neg", "-rounds -2", ()), ("growth", "-growth 0.99", ()), ("growth_nan", "-growth nan", ()),
    ("gap", "-gap -1", ()), ("growth_at_one_round", "-rounds 1 -growth 0.5", ()),
    ("two_rounds_growth", "-rounds 0 -growth 0.5", ()), ("two_growth_gap", "-growth 0.5 -gap -1", ()), ("two_gap_window", "-gap -1 -window 0", ()),
    ("two_window_minPairs", "-window 0 -minPairs -1", ()), ("two_minPairs_minSize", "-minPairs -1 -minSize -1", ()),
    ("two_minSize_minRatio", "-minSize -1 -minRatio 0.5", ()), ("two_minRatio_no_pairs", "-minRatio 0.5 -config {no_pairs}", ("more_configs",))],
    ("A", "B"), with_order=False)
CASES += [
    case("scaffoldLinks-refused-by_links_resident", "scaffoldLinks", "links_verdicts", "-config {cfg} -out {d}/links", "refusing_links"),
    case("scaffoldLinks-refused-by_links_lifted", "scaffoldLinks", "links_planted", "-config {cfg} -out {d}/links -window 5000 -rounds 2", "refusing_lifted"),
]


# ---- running one -----------------------------------------------------------------------------------------------------------------------
def _digests(d):
    out = {}
    for where, _subs, files in os.walk(d):
        for fn in files:
            path = os.path.join(where, fn)
            with open(path, "rb") as fh:
                out[os.path.relpath(path, d)] = hashlib.sha256(fh.read()).hexdigest()
    return out


def _plain(x):
    """A returned value as JSON can hold it: arrays and tuples as lists, the keys of a dict as text, in order."""
    if isinstance(x, np.ndarray):
        return _plain(x.tolist())
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, dict):
        return [[_plain(k), _plain(v)] for k, v in sorted(x.items(), key=lambda kv: repr(kv[0]))]
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def run_case(c, tmp_dir):
    """{"stdout", "exit", "returned", "files", "calls"} of a case run in the empty directory ``tmp_dir``: what the tool
    printed; the code of its SystemExit, None without one; the sha256 of what ``main`` returned, as JSON; {relative path:
    sha256} of every file the run wrote or changed under ``tmp_dir``; the methods it called on its context.  ``tmp_dir`` reads
    <TMP> in every text."""
    import importlib
    d = os.path.realpath(str(tmp_dir))
    words = SETUPS[c["setup"]](d)
    for name, text in c["files"].items():
        _write(d, name, text)
    for extra in c["extras"]:
        EXTRAS[extra](d, words)
    words = dict({k: v for k, v in words.items() if not k.startswith("_")}, d=d)
    argv = [a.format(**words) for a in c["args"]]
    tool = importlib.import_module("hic_genome_assembler_amd." + c["tool"])
    context = Recorder(CONTEXTS[c["context"]]())
    before = _digests(d)
    printed, code, returned = io.StringIO(), None, None
    keep = sys.argv[0], os.environ.get("COLUMNS")
    sys.argv[0], os.environ["COLUMNS"] = c["tool"] + ".py", "120"             # what argparse names the program and how wide it writes
    try:
        with contextlib.redirect_stdout(printed):
            try:
                returned = hashlib.sha256(json.dumps(_plain(tool.main(argv, context=context))).encode()).hexdigest()
            except SystemExit as exc:
                code = exc.code
    finally:
        sys.argv[0] = keep[0]
        if keep[1] is None:
            del os.environ["COLUMNS"]
        else:
            os.environ["COLUMNS"] = keep[1]
    after = _digests(d)
    return {"stdout": printed.getvalue().replace(d, "<TMP>"), "exit": code.replace(d, "<TMP>") if isinstance(code, str) else code,
            "returned": returned, "files": {p: h for p, h in sorted(after.items()) if before.get(p) != h}, "calls": context.called}


def record():
    import tempfile
    out = {}
    for c in CASES:
        with tempfile.TemporaryDirectory() as d:
            out[c["id"]] = run_case(c, d)
    os.makedirs(os.path.dirname(RECORD), exist_ok=True)
    with open(RECORD, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return out


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/pairtool_cases.py --record")
    print("%d cases recorded in %s" % (len(record()), os.path.relpath(RECORD, ROOT)))
