"""The end-link graph of all scaffolds from the read pairs, before any ordering exists, on the device (DESIGN.md section
9t).

Every other read-pair tool starts from an order file and counts links only where that file says to look.  This one answers
the question a Hi-C scaffolder starts from (LACHESIS, SALSA, 3D-DNA, YaHS): which scaffold ends are linked to which, over
all scaffolds.  It loads ``validPairFile`` into the resident pair store of a context once and counts, in one pass over the
store, the pairs between every two scaffolds by the end zones of ``-window`` bp their ends fall in, every scaffold read left
to right as the size file has it.  From that table it writes the links of every scaffold pair, the best and second-best
partner of every scaffold end with a verdict, the paths the reciprocal best ends form - an order file ``placeUnplaced`` and
``polishOrder`` take - and, with ``-order``, an audit of every junction of an order file against the read pairs.

    python -m hic_genome_assembler_amd.scaffoldLinks -config my_config.txt [-window 50000] [-minPairs 4] [-minRatio 2] \\
           [-minSize 0] [-order FILE] [-rounds 1] [-growth 1] [-gap 100] [-out DIR] [-threads 0] [-device 0]

With ``-rounds R`` above 1 the tool iterates as those scaffolders do: the paths of a round are the
sequences of the next, laid out as ``assembledMap`` lays out a chromosome with ``-gap`` bases between neighbours, and round
r counts the pairs between the end zones of those sequences - both ends of every stored pair lifted, one more pass over the
store - at the window of the round before times ``-growth``.  The same verdicts, ``-minPairs``, ``-minRatio`` and
``-minSize`` then apply to sequences.  The loop ends ``nothing_left`` after a round that keeps no join and ``round_limit``
after round R; a join is never undone in a later round.  Round 1 writes what it writes without the flag; round r writes
``round<r>/sequences.tsv``, ``links.tsv``, ``ends.tsv`` and ``paths.order``, and the run ``rounds.tsv`` and ``final.order``.

Verdicts of a scaffold end, checked in this order: ``too_small`` (the scaffold is below ``-minSize``: it neither chooses nor
is chosen), ``no_links``, ``weak`` (the best partner end has fewer than ``-minPairs`` pairs), ``tied`` (two ends share the
maximum), ``ambiguous`` (the best is below ``-minRatio`` times the best end of any other scaffold), ``one_sided`` (the chosen
end chose another) and ``joined`` (reciprocal).  There is no restriction-site normalisation.  The defaults are choices, not tuned values.  A ``-window`` wider than the shortest scaffolds makes
ends skip over them: a scaffold of up to two windows is all end zone, so its neighbours' ends see each other through it.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import math
import os

import numpy as np

from . import _lib, pairtool
from . import placeUnplaced as place
from .assembledMap import DEFAULT_GAP
from .orientSmallScaffolds import writeScaffoldOrderingsToFile
from .pairtool import DEFAULT_MIN_PAIRS, DEFAULT_MIN_RATIO, DEFAULT_MIN_SIZE, DEFAULT_WINDOW

MAX_SCAFFOLDS = _lib.LINKS_MAX_SCAF
END_NAMES = ("left", "right")
LINK_COLUMNS = ("scaffold_a", "scaffold_b", "pairs", "left_left", "left_right", "right_left", "right_right")
END_COLUMNS = ("scaffold", "end", "zone_bases", "links", "best_scaffold", "best_end", "best_pairs", "second_scaffold", "second_end",
               "second_pairs", "ratio", "verdict")
PATH_COLUMNS = ("path", "scaffolds", "bases", "fewest_pairs")
JUNCTION_COLUMNS = ("chromosome", "left_scaffold", "left_end", "right_scaffold", "right_end", "pairs", "left_best", "left_best_pairs",
                    "right_best", "right_best_pairs", "verdict")
CHOSE = ("one_sided", "joined")
DEFAULT_ROUNDS, DEFAULT_GROWTH = 1, 1.0
SEQUENCE_COLUMNS = ("sequence", "scaffolds", "bases", "members")
ROUND_COLUMNS = ("round", "window", "sequences_in", "rows", "linked", "middle", "inside", "unlifted", "joins", "cycles_cut",
                 "sequences_out", "paths", "singles")


def zone_bases(size, window):
    """(left zone, right zone) of a scaffold in bases: a scaffold of up to two windows is cut in halves, the left half taking
    the odd base."""
    size, window = int(size), int(window)
    return min(window, size - size // 2), min(window, size // 2)


def end_links(lo, hi, counts, n_scaf):
    """{end: {partner end: pairs}} from the rows of ``links_resident``; the end ``2 s`` is the left end of scaffold s and
    ``2 s + 1`` its right end.  Only counts above 0 are entered."""
    links = {e: {} for e in range(2 * n_scaf)}
    for a, b, row in zip(np.asarray(lo).tolist(), np.asarray(hi).tolist(), np.asarray(counts).tolist()):
        for combo in range(4):
            if row[combo]:
                ea, eb = 2 * a + combo // 2, 2 * b + combo % 2
                links[ea][eb] = links[ea].get(eb, 0) + int(row[combo])
                links[eb][ea] = links[eb].get(ea, 0) + int(row[combo])
    return links


def end_calls(links, sizes, minPairs, minRatio, minSize):
    """{end: dict} with ``links`` (pairs with every end of a scaffold that takes part), ``best`` and ``second`` as (end,
    pairs) or None, ``ratio`` (a float, inf when the second has no link, None without a best) and ``verdict``.  The best
    partner end is the highest count among the ends of other scaffolds, the lowest end number first; the second is the
    best end of any scaffold other than the best's."""
    n_scaf = len(sizes)
    small = [int(sizes[s]) < minSize for s in range(n_scaf)]
    calls = {}
    for e in range(2 * n_scaf):
        s = e // 2
        if small[s]:
            calls[e] = {"links": 0, "best": None, "second": None, "ratio": None, "verdict": "too_small"}
            continue
        partners = sorted(((x, f) for f, x in links[e].items() if f // 2 != s and not small[f // 2]), key=lambda t: (-t[0], t[1]))
        call = {"links": sum(x for x, _f in partners), "best": None, "second": None, "ratio": None}
        if not partners:
            call["verdict"] = "no_links"
            calls[e] = call
            continue
        m, best = partners[0]
        others = [(x, f) for x, f in partners if f // 2 != best // 2]
        second = others[0] if others else None
        call["best"] = (best, m)
        call["second"] = None if second is None else (second[1], second[0])
        call["ratio"] = float("inf") if second is None else m / second[0]
        if m < minPairs:
            call["verdict"] = "weak"
        elif len(partners) > 1 and partners[1][0] == m:
            call["verdict"] = "tied"
        elif second is not None and (m == second[0] or call["ratio"] < minRatio):
            call["verdict"] = "ambiguous"
        else:
            call["verdict"] = None                                # it chooses ``best``; one_sided or joined below
        calls[e] = call
    for e, call in calls.items():
        if call["verdict"] is None:
            f = call["best"][0]
            call["verdict"] = "joined" if calls[f]["verdict"] in (None, "joined") and calls[f]["best"][0] == e else "one_sided"
    return calls


def joins_of(calls):
    """[(end, end, pairs)] with the lower end first, in end order: the reciprocal choices."""
    return [(e, call["best"][0], call["best"][1]) for e, call in sorted(calls.items())
            if call["verdict"] == "joined" and e < call["best"][0]]


def paths_of(joins, sizes):
    """(paths, cycles cut, kept joins): the joins and every scaffold's own left-to-right edge form paths and cycles.  A cycle
    drops its join of fewest pairs, then the one with the lowest end number.  A path of at least two scaffolds is
    [(scaffold, "+" / "-"), ...] from its terminal scaffold of lower index; + when the path runs from the scaffold's left end
    to its right end.  Paths come by total bases descending, then by first scaffold."""
    joins = list(joins)
    cut = 0
    while True:
        mate = {}
        for a, b, x in joins:
            mate[a], mate[b] = (b, x), (a, x)
        seen, cycle = set(), None
        for a, _b, _x in joins:                                   # walk from every joined end until a free end or the start again
            if a in seen:
                continue
            members, e = [], a
            while True:
                seen.add(e)
                other = e ^ 1                                     # through the scaffold
                seen.add(other)
                if other not in mate:
                    break
                members.append((min(other, mate[other][0]), max(other, mate[other][0]), mate[other][1]))
                e = mate[other][0]
                if e == a:
                    cycle = members
                    break
            if cycle:
                break
        if not cycle:
            break
        worst = min(cycle, key=lambda j: (j[2], j[0]))
        joins.remove(worst)
        cut += 1
    mate = {}
    for a, b, x in joins:
        mate[a], mate[b] = b, a
    joined = sorted({e // 2 for e in mate})
    paths, done = [], set()
    for s in joined:
        if s in done or (2 * s in mate and 2 * s + 1 in mate):
            continue                                              # not a terminal scaffold; its path starts elsewhere
        # s is terminal: enter at its free end
        e = 2 * s if 2 * s not in mate else 2 * s + 1
        path = []
        while True:
            t = e // 2
            path.append((t, "+" if e % 2 == 0 else "-"))
            done.add(t)
            out = e ^ 1
            if out not in mate:
                break
            e = mate[out]
        if path[-1][0] < path[0][0]:                              # start at the terminal scaffold of lower index
            path = [(t, "-" if o == "+" else "+") for t, o in reversed(path)]
        paths.append(path)
    paths.sort(key=lambda p: (-sum(int(sizes[t]) for t, _o in p), p[0][0]))
    return paths, cut, joins


def fewest_pairs(path, joins):
    """The fewest pairs among the joins between the consecutive scaffolds of a path."""
    by_scaffolds = {(a // 2, b // 2): x for a, b, x in joins}
    by_scaffolds.update({(b // 2, a // 2): x for a, b, x in joins})
    return min(by_scaffolds[(path[k][0], path[k + 1][0])] for k in range(len(path) - 1))


def _end_text(names, end):
    return "NA" if end is None else "%s:%s" % (names[end // 2], END_NAMES[end % 2])


def junction_rows(asm, names, links, calls):
    """The rows of junctions.tsv: every junction and every chromosome end of an assembly with the two facing ends, their
    pairs, each end's best partner and ``agreed`` (reciprocal best), ``contested`` (an end's best, passing -minPairs and
    -minRatio, is another end; it is named) or ``open``."""
    rows = []
    for q in range(asm.n_chromosomes):
        comps = asm.components[q]
        facing = [(2 * s + (1 if o == "-" else 0), 2 * s + (0 if o == "-" else 1)) for s, _off, o in comps]   # (as-it-lies left, right)
        sides = [(None, facing[0][0])] + [(facing[k][1], facing[k + 1][0]) for k in range(len(comps) - 1)] + [(facing[-1][1], None)]
        for left, right in sides:
            best = {e: (calls[e]["best"] if e is not None else None) for e in (left, right)}
            cols = [str(q + 1)]
            for e in (left, right):
                cols += ["NA", "NA"] if e is None else [names[e // 2], END_NAMES[e % 2]]
            cols.append("NA" if left is None or right is None else str(links[left].get(right, 0)))
            for e in (left, right):
                cols += ["NA", "NA"] if not best[e] else [_end_text(names, best[e][0]), str(best[e][1])]
            other = {left: right, right: left}
            rivals = [calls[e]["best"][0] for e in (left, right)
                      if e is not None and calls[e]["verdict"] in CHOSE and calls[e]["best"][0] != other[e]]
            if left is not None and right is not None and best[left] and best[right] and best[left][0] == right and best[right][0] == left \
                    and calls[left]["verdict"] != "tied" and calls[right]["verdict"] != "tied":
                verdict = "agreed"
            elif rivals:
                verdict = "contested:" + ",".join(_end_text(names, f) for f in rivals)
            else:
                verdict = "open"
            rows.append(cols + [verdict])
    return rows


def decide(lo, hi, counts, sizes, minPairs, minRatio, minSize):
    """(links, calls, all joins, paths, cycles cut, kept joins) of one round from its rows and the sizes of its units."""
    links = end_links(lo, hi, counts, len(sizes))
    calls = end_calls(links, sizes, minPairs, minRatio, minSize)
    all_joins = joins_of(calls)
    return (links, calls, all_joins) + paths_of(all_joins, sizes)


# ---- the later rounds: the paths of one round are the sequences of the next -------------------------------------
def expand_paths(sequences, paths):
    """The sequences after a round, each [(scaffold, "+" / "-"), ...]: a path of sequences is expanded to scaffolds - a sequence
    entered as ``-`` has its scaffolds in reverse order and every orientation flipped - and turned so that it starts at its
    terminal scaffold of lower index; a sequence no path names stays as it is.  They are numbered by their first scaffold."""
    flip = {"+": "-", "-": "+"}
    out, used = [], set()
    for path in paths:
        members = []
        for q, o in path:
            used.add(q)
            members += sequences[q] if o == "+" else [(s, flip[p]) for s, p in reversed(sequences[q])]
        if members[-1][0] < members[0][0]:
            members = [(s, flip[p]) for s, p in reversed(members)]
        out.append(members)
    out += [list(members) for q, members in enumerate(sequences) if q not in used]
    return sorted(out, key=lambda members: members[0][0])


def sequence_tables(sequences, sizes, gap):
    """(lift_seq int32, lift_off int64, lift_rev uint8, seq_sizes int64) of the sequences laid out as assembledMap lays out a
    chromosome: offsets from 0 and ``gap`` bases between neighbours.  Every scaffold lies in one sequence."""
    n_scaf = len(sizes)
    seq, off, rev = np.full(n_scaf, -1, np.int32), np.zeros(n_scaf, np.int64), np.zeros(n_scaf, np.uint8)
    seq_sizes = np.zeros(len(sequences), np.int64)
    for q, members in enumerate(sequences):
        at = 0
        for k, (s, o) in enumerate(members):
            at += gap if k else 0
            seq[s], off[s], rev[s] = q, at, o == "-"
            at += int(sizes[s])
        seq_sizes[q] = at
    assert np.all(seq >= 0)
    return seq, off, rev, seq_sizes


def layout_paths(sequences, sizes):
    """The sequences of two or more scaffolds as an order file has them: by scaffold bases descending, then by first scaffold."""
    return sorted((m for m in sequences if len(m) > 1), key=lambda m: (-sum(int(sizes[s]) for s, _o in m), m[0][0]))


def next_window(window, growth):
    """floor(window x growth), kept inside 64 bits: beyond every sequence all windows are one."""
    return min(int(math.floor(window * growth)), 1 << 62)


def later_rounds(ctx, names, sizes, first_paths, window, rounds, growth, gap, minPairs, minRatio, minSize):
    """Rounds 2 .. ``rounds`` on the resident store of ``ctx``, from the paths of round 1.  Returns (per-round dicts, how the
    loop ended, the last sequences).  A round dict holds everything its files are written from."""
    sequences = expand_paths([[(s, "+")] for s in range(len(names))], first_paths)
    done, joined = [], len(first_paths) > 0
    for r in range(2, rounds + 1):
        if not joined:
            break
        window = next_window(window, growth)
        tables = sequence_tables(sequences, sizes, gap)
        lo, hi, counts, counters = ctx.links_lifted(sizes, *tables, window)
        links, calls, all_joins, paths, cut, joins = decide(lo, hi, counts, tables[3], minPairs, minRatio, minSize)
        after = expand_paths(sequences, paths)
        done.append({"round": r, "window": window, "sequences": sequences, "seq_sizes": tables[3], "lo": lo, "hi": hi, "counts": counts,
                     "counters": counters, "calls": calls, "all_joins": all_joins, "cut": cut, "after": after})
        sequences, joined = after, len(joins) > 0
    ended = "round_limit" if joined else "nothing_left"
    return done, ended, sequences


def table_texts(labels, sizes, window, lo, hi, counts, calls):
    """The lines of links.tsv and of ends.tsv for units - scaffolds, or the sequences of a later round - of these labels and sizes."""
    link_text = ["#" + "\t".join(LINK_COLUMNS) + "\n"]
    for a, b, row in zip(lo.tolist(), hi.tolist(), counts.tolist()):
        link_text.append("\t".join([labels[a], labels[b], str(sum(row))] + [str(x) for x in row[:4]]) + "\n")
    end_text = ["#" + "\t".join(END_COLUMNS) + "\n"]
    for e in range(2 * len(labels)):
        call = calls[e]
        cols = [labels[e // 2], END_NAMES[e % 2], str(zone_bases(sizes[e // 2], window)[e % 2]), str(call["links"])]
        for which in ("best", "second"):
            cols += ["NA", "NA", "NA"] if call[which] is None else [labels[call[which][0] // 2], END_NAMES[call[which][0] % 2], str(call[which][1])]
        end_text.append("\t".join(cols + [place._ratio_text(call["ratio"]), call["verdict"]]) + "\n")
    return link_text, end_text


def write_order(path, names, sequences, sizes):
    with contextlib.redirect_stdout(io.StringIO()):               # the writer reports what it wrote; this tool prints its own lines
        writeScaffoldOrderingsToFile([[[names[s], o] for s, o in m] for m in layout_paths(sequences, sizes)], path)


def write_rounds(outDir, names, sizes, first, done, ended, sequences):
    """round<r>/ of every later round, rounds.tsv and final.order; one printed line per later round and a closing one."""
    lines = ["#" + "\t".join(ROUND_COLUMNS) + "\n"]
    for rnd in [first] + done:
        r, after = rnd["round"], rnd["after"]
        n_paths = sum(len(m) > 1 for m in after)
        lines.append("\t".join(str(x) for x in [r, rnd["window"], len(rnd["sequences"]), len(rnd["lo"])] + [int(x) for x in rnd["counters"]]
                               + [len(rnd["all_joins"]), rnd["cut"], len(after), n_paths, len(after) - n_paths]) + "\n")
        if r == 1:
            continue
        labels = ["seq_%d" % (q + 1) for q in range(len(rnd["sequences"]))]
        seq_text = ["#" + "\t".join(SEQUENCE_COLUMNS) + "\n"]
        for label, members, bases in zip(labels, rnd["sequences"], rnd["seq_sizes"].tolist()):
            seq_text.append("%s\t%d\t%d\t%s\n" % (label, len(members), bases, ",".join(names[s] + o for s, o in members)))
        link_text, end_text = table_texts(labels, rnd["seq_sizes"], rnd["window"], rnd["lo"], rnd["hi"], rnd["counts"], rnd["calls"])
        where = os.path.join(outDir, "round%d" % r)
        os.makedirs(where, exist_ok=True)
        for fn, text in (("sequences.tsv", seq_text), ("links.tsv", link_text), ("ends.tsv", end_text)):
            pairtool.write_text(os.path.join(where, fn), "".join(text))
        write_order(os.path.join(where, "paths.order"), names, after, sizes)
        print("LINKS round %d: window %d, sequences %d, rows %d, joins %d, sequences out %d"
              % (r, rnd["window"], len(rnd["sequences"]), len(rnd["lo"]), len(rnd["all_joins"]), len(after)))
    lines.append("#ended=%s\n" % ended)
    pairtool.write_text(os.path.join(outDir, "rounds.tsv"), "".join(lines))
    write_order(os.path.join(outDir, "final.order"), names, sequences, sizes)
    n_paths = sum(len(m) > 1 for m in sequences)
    print("LINKS: %d rounds, ended %s, paths %d, singles %d" % (1 + len(done), ended, n_paths, len(sequences) - n_paths))


def runPipeline(configFile, window=DEFAULT_WINDOW, minPairs=DEFAULT_MIN_PAIRS, minRatio=DEFAULT_MIN_RATIO, minSize=DEFAULT_MIN_SIZE,
                orderFile=None, outDir=None, threads=0, device=0, context=None, rounds=DEFAULT_ROUNDS, growth=DEFAULT_GROWTH,
                gap=DEFAULT_GAP):
    """``context``: a context of the caller's that has ``pairs_file``, ``pairs_info``, ``links_resident`` and ``pairs_drop``
    (and ``links_lifted`` when ``rounds`` is above 1); None: a context of its own on ``device``.  Either way the file is
    loaded into the resident pair store once, counted in one call per round and the store dropped.  Returns (stats4, joins
    [(end name, end name, pairs)], paths [[(name, orientation)]]) of round 1."""
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    if outDir is None:
        outDir = os.path.join(v["saveFilesDirectory"], "links")
    with pairtool.refusing(OSError, ValueError):
        if rounds < 1:
            raise ValueError("rounds %d is below 1" % rounds)
        if not growth >= 1:
            raise ValueError("growth %g is below 1" % growth)
        if gap < 0:
            raise ValueError("gap %d is negative" % gap)
        pairtool.check_thresholds(window=window, minPairs=minPairs, minSize=minSize, minRatio=minRatio)
        names, sizes = pairtool.read_scaffolds(v)
        if len(names) > MAX_SCAFFOLDS:
            raise ValueError("%d scaffolds, more than the %d a link key has room for" % (len(names), MAX_SCAFFOLDS))
        asm = None
        if pairtool.resolve_order(v, orderFile, default=False) is not None:
            asm = pairtool.order_assembly(orderFile, names, sizes)
    n_scaf = len(names)

    made = {"decided": None, "later": None}

    def count(ctx):
        stats = tuple(ctx.pairs_file(v["validPairFile"], names, sizes, threads=threads)[:4])
        try:
            n_kept, n_intra = ctx.pairs_info()[:2]
            first = tuple(ctx.links_resident(sizes, window))
            if rounds > 1:                                        # the later rounds need the store; every file is written below
                made["decided"] = decide(first[0], first[1], first[2], sizes, minPairs, minRatio, minSize)
                made["later"] = later_rounds(ctx, names, sizes, made["decided"][3], window, rounds, growth, gap, minPairs, minRatio,
                                             minSize)
            return (stats, int(n_kept), int(n_intra)) + first
        finally:
            ctx.pairs_drop()

    stats, n_kept, n_intra, lo, hi, counts, counters = pairtool.on_context(context, device, count)
    if int(counts.sum()) != n_kept or int(counters.sum()) != n_kept:
        pairtool.refuse("the rows hold %d pairs and the counters %d where the store kept %d" % (int(counts.sum()), int(counters.sum()), n_kept))
    for rnd in made["later"][0] if made["later"] else ():
        if int(rnd["counters"].sum()) != n_kept or int(rnd["counts"].sum()) != int(rnd["counters"][:2].sum()):
            pairtool.refuse("round %d: the rows hold %d pairs and the counters %d where the store kept %d"
                            % (rnd["round"], int(rnd["counts"].sum()), int(rnd["counters"].sum()), n_kept))

    links, calls, all_joins, paths, cut, joins = made["decided"] or decide(lo, hi, counts, sizes, minPairs, minRatio, minSize)
    in_paths = sum(len(p) for p in paths)
    header = ["window=%d" % window, "minPairs=%d" % minPairs, "minRatio=%g" % minRatio, "minSize=%d" % minSize]
    header += pairtool.fields(pairtool.STATS_COLUMNS, stats)
    header += ["pairs_kept=%d" % n_kept, "pairs_intra=%d" % n_intra, "linked=%d" % int(counters[0]), "middle=%d" % int(counters[1]),
               "rows=%d" % len(lo), "joins=%d" % len(all_joins), "cycles_cut=%d" % cut, "paths=%d" % len(paths),
               "singles=%d" % (n_scaf - in_paths)]

    link_text, end_text = table_texts(names, sizes, window, lo, hi, counts, calls)
    summary = ["#" + "\t".join(header) + "\n", "#" + "\t".join(PATH_COLUMNS) + "\n"]
    for k, path in enumerate(paths, 1):
        summary.append("%d\t%d\t%d\t%d\n" % (k, len(path), sum(int(sizes[t]) for t, _o in path), fewest_pairs(path, joins)))
    junction_text = None
    if asm is not None:
        junction_text = ["#" + "\t".join(JUNCTION_COLUMNS) + "\n"] + ["\t".join(r) + "\n" for r in junction_rows(asm, names, links, calls)]

    os.makedirs(outDir, exist_ok=True)
    for fn, text in (("links.tsv", link_text), ("ends.tsv", end_text), ("links_summary.tsv", summary), ("junctions.tsv", junction_text)):
        if text is not None:
            pairtool.write_text(os.path.join(outDir, fn), "".join(text))
    with contextlib.redirect_stdout(io.StringIO()):               # the writer reports what it wrote; this tool prints one line
        writeScaffoldOrderingsToFile([[[names[t], o] for t, o in path] for path in paths], os.path.join(outDir, "paths.order"))
    print("LINKS: scaffolds %d, pairs kept %d, rows %d, joins %d, paths %d" % (n_scaf, n_kept, len(lo), len(all_joins), len(paths)))
    if made["later"]:
        first = {"round": 1, "window": window, "sequences": [[(s, "+")] for s in range(n_scaf)], "lo": lo,
                 "counters": [int(counters[0]), int(counters[1]), 0, 0], "all_joins": all_joins, "cut": cut,
                 "after": expand_paths([[(s, "+")] for s in range(n_scaf)], paths)}
        write_rounds(outDir, names, sizes, first, *made["later"])
    return (stats, [(_end_text(names, a), _end_text(names, b), x) for a, b, x in all_joins],
            [[(names[t], o) for t, o in path] for path in paths])


def main(argv=None, context=None):
    parser = argparse.ArgumentParser(description="Counts, on the GPU, the read pairs of validPairFile between the end zones of "
                                                 "every two scaffolds, without an order file, and writes the link table, the best "
                                                 "partner of every scaffold end and the paths the reciprocal best ends form.")
    with pairtool.common_arguments(parser, order=False):
        parser.add_argument("-window", help="End zone of a scaffold in bp (default %d)" % DEFAULT_WINDOW, type=int, default=DEFAULT_WINDOW)
        parser.add_argument("-minPairs", help="Pairs below which an end chooses no partner (default %d)" % DEFAULT_MIN_PAIRS, type=int,
                            default=DEFAULT_MIN_PAIRS)
        parser.add_argument("-minRatio", help="Pairs of the best partner end over the best end of any other scaffold below which an end "
                                              "chooses none (default %g)" % DEFAULT_MIN_RATIO, type=float, default=DEFAULT_MIN_RATIO)
        parser.add_argument("-minSize", help="Scaffolds below this size neither choose nor are chosen (default %d)" % DEFAULT_MIN_SIZE,
                            type=int, default=DEFAULT_MIN_SIZE)
        parser.add_argument("-order", help="Audit the junctions of this order file against the links (junctions.tsv); it is never changed",
                            type=str, default=None)
        parser.add_argument("-rounds", help="Rounds at the most: from round 2 on the paths of the round before are the units, their links "
                                            "counted between lifted ends (default %d: a single round)" % DEFAULT_ROUNDS, type=int,
                            default=DEFAULT_ROUNDS)
        parser.add_argument("-growth", help="Factor of at least 1 by which -window grows from a round to the next (default %g)"
                                            % DEFAULT_GROWTH, type=float, default=DEFAULT_GROWTH)
        parser.add_argument("-gap", help="Bases between neighbouring scaffolds of a sequence of a later round (default %d, as assembledMap)"
                                         % DEFAULT_GAP, type=int, default=DEFAULT_GAP)
        parser.add_argument("-out", help="Directory of the results (default: saveFilesDirectory/links)", type=str, default=None)
    args = parser.parse_args(argv)
    return runPipeline(args.config, args.window, args.minPairs, args.minRatio, args.minSize, args.order, args.out, threads=args.threads,
                       device=args.device, context=context, rounds=args.rounds, growth=args.growth, gap=args.gap)


if __name__ == "__main__":
    main()
