"""The front end of the tools that read ``validPairFile`` against an order file - supportSpans, supportEnds, placeUnplaced,
supportSeats, polishOrder and scaffoldLinks: the refusal, the checks of the arguments they share, the
inputs loaded in steps, the block that runs on the caller's context or on one of the run's own, the host chunk loop, the
order file read and written again byte for byte, and the pieces of their reports.  What only one tool does is in that tool.
"""
from __future__ import annotations

import contextlib
import os
import sys

from . import _lib
from .assembledMap import DEFAULT_GAP, build_assembly, read_order_file
from .buildMap import STATS_COLUMNS, check_valid_pair_file  # noqa: F401  (STATS_COLUMNS: for the tools)
from .hostio import paused_gc, read_scaffold_sizes

DEFAULT_WINDOW, DEFAULT_REACH, DEFAULT_MIN_PAIRS, DEFAULT_MIN_RATIO, DEFAULT_MIN_SIZE = 50000, 2, 4, 2.0, 0
MAX_REACH = 64
MAX_TABLE = 1 << 27
CHUNK_PAIRS = 1 << 22


# ---- refusals and arguments --------------------------------------------------------------------------------------------------------
def refuse(exc):
    sys.exit("ERROR... %s. Exiting..." % exc)


@contextlib.contextmanager
def refusing(*errors):
    """Inside, an error of one of these kinds ends the run through ``refuse``."""
    try:
        yield
    except errors as exc:
        refuse(exc)


def check_thresholds(window=None, reach=None, minPairs=None, minSize=None, minRatio=None):
    """ValueError for the first of the arguments a tool has, in this order, that is out of range."""
    if window is not None and window < 1:
        raise ValueError("the window %d is below 1" % window)
    if reach is not None and not 1 <= reach <= MAX_REACH:
        raise ValueError("the reach %d is outside 1 .. %d" % (reach, MAX_REACH))
    if minPairs is not None and minPairs < 0:
        raise ValueError("minPairs %d is negative" % minPairs)
    if minSize is not None and minSize < 0:
        raise ValueError("minSize %d is negative" % minSize)
    if minRatio is not None and not minRatio >= 1:
        raise ValueError("minRatio %g is below 1" % minRatio)


@contextlib.contextmanager
def common_arguments(parser, order=True):
    """-config and -order in front of the arguments a tool adds inside, -threads and -device behind them."""
    parser.add_argument("-config", help="Full file path to the config file", required=True, type=str)
    if order:
        parser.add_argument("-order", help="Order file (default: finalOrderingsFile when it exists, else chromosomeOrderFile)",
                            type=str, default=None)
    yield parser
    parser.add_argument("-threads", help="Host threads of the parser (default 0: all)", type=int, default=0)
    parser.add_argument("-device", help="GPU index (default 0)", type=int, default=0)


# ---- the inputs, in steps: a tool may have a check of its own between two of them ------------------------------------------------------
def read_scaffolds(v):
    """(names, sizes) of hicProScaffSizeFile, after validPairFile is found to be a file of read pairs."""
    check_valid_pair_file(v["validPairFile"])
    names, sizes = read_scaffold_sizes(v["hicProScaffSizeFile"])
    if not names:
        raise ValueError("hicProScaffSizeFile %s lists no scaffold" % v["hicProScaffSizeFile"])
    return names, sizes


def resolve_order(v, orderFile, default=True):
    """The order file of a run: the one given, with ``default`` else finalOrderingsFile when it exists, else
    chromosomeOrderFile.  None stays None without ``default``."""
    if orderFile is None and default:
        orderFile = v["finalOrderingsFile"] if os.path.isfile(v["finalOrderingsFile"]) else v["chromosomeOrderFile"]
    if orderFile is not None and not os.path.isfile(orderFile):
        raise ValueError("order file %r does not exist" % orderFile)
    return orderFile


def order_assembly(orderFile, names, sizes, gap=DEFAULT_GAP, chromosomes_only=True):
    return build_assembly(read_order_file(orderFile), names, sizes, gap, chromosomes_only=chromosomes_only)


def load(v, orderFile):
    """(names, sizes, order file, assembly of its chromosomes): the three steps of a tool that has nothing between them."""
    names, sizes = read_scaffolds(v)
    orderFile = resolve_order(v, orderFile)
    return names, sizes, orderFile, order_assembly(orderFile, names, sizes)


# ---- the device -------------------------------------------------------------------------------------------------------------------------
def on_context(context, device, work):
    """``work(ctx)`` on the caller's ``context``, or with None on a context of the run's own on ``device`` that is closed after
    it; the collector is paused and a HicmiError refused.  Which call ``work`` makes on which kind of context is the tool's."""
    with paused_gc(), refusing(_lib.HicmiError):
        if context is not None:
            return work(context)
        with _lib.Context(device) as ctx:
            return work(ctx)


def parse_in_chunks(pairFile, names, sizes, threads, add_pairs):
    """stats4 of ``pairFile`` parsed on the host in chunks (hicmi_parse_valid_pairs), each handed to ``add_pairs(sa, pa, sb, pb)``."""
    stats, at, size = [0, 0, 0, 0], 0, os.path.getsize(pairFile)
    while True:
        room = max(1, (size - at) // 12 + 1)                                   # a six-column line has 12 bytes or more
        sa, pa, sb, pb, at, st = _lib.parse_valid_pairs(pairFile, names, sizes, first_byte=at, max_pairs=min(CHUNK_PAIRS, room),
                                                        threads=threads)
        stats = [a + b for a, b in zip(stats, st)]
        add_pairs(sa, pa, sb, pb)
        if at >= size:
            return tuple(stats)


# ---- the order file, byte for byte -----------------------------------------------------------------------------------------------------
def order_lines(orderFile):
    """[(line, body, ending, name)] of an order file: every line as it stands, without its line ending, the ending, and the
    scaffold it names - None for the first line, an empty line and a comment."""
    with open(orderFile, newline="") as fh:
        lines = list(fh)
    bodies = [line.rstrip("\r\n") for line in lines]
    return [(line, body, line[len(body):], body.split("\t")[0] if k and body and body[0] != "#" else None)
            for k, (line, body) in enumerate(zip(lines, bodies))]


def _signed(body, ending, sign):
    cols = body.split("\t")
    cols[1] = sign
    return "\t".join(cols) + ending


def flipped_order_text(orderFile, flips):
    """The order file again, every line verbatim except that the sign of each scaffold of ``flips`` is changed."""
    return "".join(_signed(body, ending, "+" if body.split("\t")[1] == "-" else "-") if name in flips else line
                   for line, body, ending, name in order_lines(orderFile))


def placed_order_text(orderFile, insertions):
    """The order file again, every line verbatim, with a line ``name<TAB>orientation`` per entry of ``insertions``:
    {scaffold the line goes before: (name, orientation)} and {(scaffold the line goes after, None): (name, orientation)}.
    The new line takes the line ending of the line it is placed next to."""
    out = []
    for line, body, ending, name in order_lines(orderFile):
        if name is not None and name in insertions:
            out.append("%s\t%s" % insertions[name] + (ending or "\n"))
        out.append(line)
        if name is not None and (name, None) in insertions:
            if not ending:
                out[-1] = body + "\n"
            out.append("%s\t%s" % insertions[(name, None)] + ending)
    return "".join(out)


def moved_order_text(orderFile, moves):
    """The order file again with the line of every scaffold of ``moves`` - {name: (where, orientation)} - taken out and put
    back before the line of the scaffold ``where``, or after it when ``where`` is (name, None), its sign set to
    ``orientation``.  Every other byte of every line is kept; a file without a final newline stays one."""
    rows = order_lines(orderFile)
    taken = {name: _signed(body, ending, moves[name][1]) for _line, body, ending, name in rows if name in moves}
    before = {where: name for name, (where, _o) in moves.items() if not isinstance(where, tuple)}
    after = {where[0]: name for name, (where, _o) in moves.items() if isinstance(where, tuple)}
    out = []
    for line, _body, _ending, name in rows:
        if name in taken:
            continue
        if name is not None and name in before:
            out.append(taken[before[name]])
        out.append(line)
        if name is not None and name in after:
            out.append(taken[after[name]])
    # the one line without an ending was the last one: inside the file it takes its neighbour's, and the new last line has none
    final = bool(rows) and rows[-1][2] != ""
    for k, line in enumerate(out):
        body = line.rstrip("\r\n")
        if k < len(out) - 1 and body == line:
            nxt = out[k + 1]
            out[k] = body + (nxt[len(nxt.rstrip("\r\n")):] or "\n")
        elif k == len(out) - 1 and not final:
            out[k] = body
    return "".join(out)


# ---- report pieces -------------------------------------------------------------------------------------------------------------------------
def fields(columns, values, prefix=""):
    """["column=value"] of the header line of a report: the statistics of the file with STATS_COLUMNS, a tool's counters."""
    return ["%s%s=%d" % (prefix, c, x) for c, x in zip(columns, values)]


def counted(columns, counters):
    return ", ".join("%s %d" % kv for kv in zip(columns, counters.tolist()))


def lines_line(tag, stats):
    return "%s: lines %d, pairs used %d, unknown scaffold %d, out of range %d" % ((tag,) + tuple(stats))


def write_text(path, text, newline=None, mkdir=False):
    """``text`` written to ``path``; ``newline=""`` keeps its line endings, ``mkdir`` makes the directory first."""
    if mkdir:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline=newline) as fh:
        fh.write(text)


def gap_neighbours(names, members, g):
    """(left, right) of gap g of a chromosome of these members by name; ``start`` and ``end`` beyond them."""
    return names[members[g - 1]] if g else "start", names[members[g]] if g < len(members) else "end"


def write_gap_tables(fullDir, prefix, names, n_seq, links, gaps):
    """``prefix``.chromosomes.tsv from ``links`` [(scaffold, links with every chromosome)] and ``prefix``.gaps.tsv from ``gaps``
    [(scaffold, its chromosome, the members the gaps lie between, scores[g][o])], in ``fullDir``."""
    text = ["#scaffold\t" + "\t".join("Chr_%d" % (q + 1) for q in range(n_seq)) + "\n"]
    text += [names[s] + "\t" + "\t".join(str(x) for x in a) + "\n" for s, a in links]
    write_text(os.path.join(fullDir, prefix + ".chromosomes.tsv"), "".join(text), mkdir=True)
    text = ["#scaffold\tchromosome\tgap\tleft\tright\torientation\tscore\n"]
    for s, q, members, scores in gaps:
        text += ["%s\t%d\t%d\t%s\t%s\t%s\t%d\n" % ((names[s], q + 1, g) + gap_neighbours(names, members, g) + ("+-"[o], x))
                 for g, both in enumerate(scores) for o, x in enumerate(both)]
    write_text(os.path.join(fullDir, prefix + ".gaps.tsv"), "".join(text), mkdir=True)
