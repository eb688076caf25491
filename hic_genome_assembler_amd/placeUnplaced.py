"""Placing the scaffolds an ordering leaves out, from their read-pair links, on the device.

Every other tool improves or questions the scaffolds an order file already names.  The ones it does not name - dropped by
Part 1, masked by Part 0, too small for a bin - end as loose sequences.  This one reads ``validPairFile`` itself, twice on
one context.  Pass 1 counts, for every unplaced scaffold, the read pairs it shares with every chromosome, and gives it to
the chromosome it is linked to most densely (links per placed base), when that one stands out.  Pass 2 counts the pairs of
each assigned scaffold against the end zones of ``-window`` bp of the scaffolds of its chromosome, separately for its own
two halves, and scores every gap of the chromosome in both orientations from the zones that face the gap, up to
``-reach`` scaffolds away.

    python -m hic_genome_assembler_amd.placeUnplaced -config my_config.txt [-order FILE] [-window 50000] [-reach 2] [-minPairs 4] \\
           [-minRatio 2] [-minSize 0] [-out FILE] [-placed FILE] [-full DIR] [-threads 0] [-device 0]

Verdicts: ``too_small`` (below ``-minSize``), ``no_links``, ``ambiguous`` (fewer than ``-minPairs`` links with the densest
chromosome, a tie with the second densest, or a density ratio below ``-minRatio``), ``chromosome_only`` (a chromosome, but
the best gap score is below ``-minPairs`` or shared by two gaps), ``placed``, ``orientation_open`` (placed as ``+``: both
orientations of the gap score the same) and ``deferred`` (another scaffold with a higher score, or the same score and an
earlier line in the size file, chose the same gap).  ``-placed`` writes the order file again with one scaffold inserted per
gap: run the tool again on that file to place the deferred ones.  A gap at the start or the end of a chromosome has
neighbours on one side only, and its score is not scaled up for it.  There is no restriction-site normalisation.  The
defaults are choices, not tuned values.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import _lib, pairtool
from .pairtool import (DEFAULT_MIN_PAIRS, DEFAULT_MIN_RATIO, DEFAULT_MIN_SIZE, DEFAULT_REACH, DEFAULT_WINDOW, MAX_REACH,  # noqa: F401
                       MAX_TABLE, placed_order_text)

COUNTER_COLUMNS = ("anchored", "middle", "elsewhere", "skipped", "unplaced", "placed")
UNPLACED_COLUMNS = ("scaffold", "size", "links", "chromosome", "chrom_links", "second", "second_links", "ratio", "left", "right",
                    "orientation", "score", "runner_up", "verdict")
CHROMOSOME_COLUMNS = ("chromosome", "scaffolds", "bases", "assigned", "inserted")
LEFT, RIGHT = 0, 1                               # end zones of a placed scaffold as it lies


def number_blocks(asm, sizes, target=None):
    """(first int64[S], n_table) of DESIGN.md 9q from the components of the assembly: the candidates in size-file order,
    a block of one counter per sequence each, or with ``target`` of four per scaffold with a base of the target."""
    filled = [sum(1 for s, _off, _o in comps if sizes[s] > 0) for comps in asm.components]
    first = np.full(len(sizes), -1, np.int64)
    n = 0
    for s in range(len(sizes)):
        if asm.lift_seq[s] < 0 and sizes[s] > 0 and (target is None or target[s] >= 0):
            first[s] = n
            n += len(asm.components) if target is None else 4 * filled[target[s]]
    return first, n


def densest(a, B):
    """(best, second) of the sequences by links per base, a[q] / B[q], compared by cross-multiplication; a tie goes to the
    lowest q, and second is None with one sequence."""
    def first_max(skip):
        top = None
        for q in range(len(a)):
            if q != skip and (top is None or a[q] * B[top] > a[top] * B[q]):
                top = q
        return top
    best = first_max(None)
    return best, first_max(best)


def choose_chromosome(a, B, size, minPairs, minRatio, minSize):
    """(best, second, ratio, verdict) of a candidate with the links a[q]; the verdict is None when it gets ``best`` as its
    target.  ratio: a float, inf when the second densest sequence has no link, None with one sequence."""
    best, second = densest(a, B)
    ratio = None
    if second is not None:
        ratio = float("inf") if a[second] == 0 else (a[best] * B[second]) / (a[second] * B[best]) if a[best] else 0.0
    if size < minSize:
        return best, second, ratio, "too_small"
    if sum(a) == 0:
        return best, second, ratio, "no_links"
    if a[best] < minPairs:
        return best, second, ratio, "ambiguous"
    if second is not None and (a[best] * B[second] == a[second] * B[best] or ratio < minRatio):
        return best, second, ratio, "ambiguous"
    return best, second, ratio, None


def gap_scores(T, reach):
    """scores[g][o] of the gaps g = 0 .. S of a chromosome of S scaffolds and the orientations o = 0 (+) and 1 (-), from the
    candidate's counters T[k, half, zone]."""
    S = T.shape[0]
    scores = []
    for g in range(S + 1):
        both = []
        for o in (0, 1):
            near, far = (0, 1) if o == 0 else (1, 0)               # the half that lies left, the half that lies right
            x = sum(int(T[g - d, near, RIGHT]) for d in range(1, reach + 1) if g - d >= 0)
            x += sum(int(T[g + d - 1, far, LEFT]) for d in range(1, reach + 1) if g + d - 1 < S)
            both.append(x)
        scores.append(both)
    return scores


def choose_gap(scores, minPairs):
    """(gap, orientation, score, runner_up, verdict): the first maximum in the order gap 0 +, gap 0 -, gap 1 +, ..., the best
    score anywhere else, and ``chromosome_only``, ``placed`` or ``orientation_open``."""
    flat = [(x, g, o) for g, both in enumerate(scores) for o, x in enumerate(both)]
    m = max(x for x, _g, _o in flat)
    at = [(g, o) for x, g, o in flat if x == m]
    g, o = at[0]
    runner_up = max(x for x, gg, oo in flat if (gg, oo) != (g, o))
    if m < minPairs or any(gg != g for gg, _o in at):
        return g, o, m, runner_up, "chromosome_only"
    return g, o, m, runner_up, "placed" if len(at) == 1 else "orientation_open"


def chromosome_members(asm, sizes):
    """(filled, B): per chromosome its scaffolds that have a base, in the order they lie, and the bases they have."""
    filled = [[s for s, _off, _o in comps if sizes[s] > 0] for comps in asm.components]
    return filled, [sum(int(sizes[s]) for s in members) for members in filled]


def both_passes(count, asm, sizes, first1, n1, minPairs, minRatio, minSize):
    """The two passes of a run over ``count(target, first, n_table)`` -> (stats4, table, counters), which counts one pass
    from the file or from a resident store: (stats4, counters of pass 1, counters of pass 2, links {s: a[q]},
    chosen {s: choose_chromosome}, T {s: [k, half, zone]})."""
    n_seq = len(asm.components)
    candidates = np.flatnonzero(first1 >= 0).tolist()
    filled, B = chromosome_members(asm, sizes)
    stats, table, counters1 = count(None, first1, n1)
    links = {s: [int(x) for x in table[first1[s]:first1[s] + n_seq]] for s in candidates}
    chosen = {s: choose_chromosome(links[s], B, int(sizes[s]), minPairs, minRatio, minSize) for s in candidates}
    target = np.full(len(sizes), -1, np.int32)
    for s, (best, _second, _ratio, verdict) in chosen.items():
        if verdict is None:
            target[s] = best
    if not (target >= 0).any():                                # no scaffold got a chromosome: there is no second pass
        return stats, counters1, np.zeros(6, np.uint64), links, chosen, {}
    first2, n2 = number_blocks(asm, sizes, target)
    if n2 > MAX_TABLE:
        pairtool.refuse("the %d scaffolds that got a chromosome need a table of %d counters, more than the %d a build can have: "
                        "raise -minSize" % (int((target >= 0).sum()), n2, MAX_TABLE))
    stats2, table, counters2 = count(target, first2, n2)
    if stats2 != stats:
        pairtool.refuse("validPairFile changed between the two passes")
    T = {s: table[first2[s]:first2[s] + 4 * len(filled[target[s]])].reshape(-1, 2, 2) for s in np.flatnonzero(target >= 0).tolist()}
    return stats, counters1, counters2, links, chosen, T


def settle_gaps(T, chosen, candidates, reach, minPairs):
    """(scores, gaps, verdicts, winners): the gap of every scaffold that got a chromosome, then one winner per gap - the
    highest score, then the lowest index - and ``deferred`` for the others that chose it."""
    scores = {s: gap_scores(T[s], reach) for s in T}
    gaps = {s: choose_gap(scores[s], minPairs) for s in T}
    verdicts = {s: chosen[s][3] or gaps[s][4] for s in candidates}
    winners = {}
    for s in sorted(gaps):
        g, _o, m, _runner_up, verdict = gaps[s]
        key = (chosen[s][0], g)
        if verdict != "chromosome_only" and (key not in winners or m > gaps[winners[key]][2]):
            winners[key] = s
    for s, (g, _o, _m, _runner_up, verdict) in gaps.items():
        if verdict != "chromosome_only" and winners[(chosen[s][0], g)] != s:
            verdicts[s] = "deferred"
    return scores, gaps, verdicts, winners


def winner_insertions(winners, gaps, filled, names):
    """The winners as ``placed_order_text`` takes them."""
    insertions = {}
    for (q, g), s in winners.items():
        members = filled[q]
        where = names[members[g]] if g < len(members) else (names[members[-1]], None)
        insertions[where] = (names[s], "+-"[gaps[s][1]])
    return insertions


def measure(ctx, pairFile, names, sizes, asm, target, window, threads):
    """(stats4, first, table, counters) through the array calls of a context the caller owns: the file is parsed on the host
    in chunks (hicmi_parse_valid_pairs) and counted chunk by chunk."""
    first = ctx.anchor_begin(sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, target, window)
    stats = pairtool.parse_in_chunks(pairFile, names, sizes, threads, ctx.anchor_add_pairs)
    table, counters = ctx.anchor_finish()
    return stats, first, table, counters


def _ratio_text(ratio):
    return "NA" if ratio is None else "inf" if ratio == float("inf") else "%.6g" % ratio


def runPipeline(configFile, orderFile=None, window=DEFAULT_WINDOW, reach=DEFAULT_REACH, minPairs=DEFAULT_MIN_PAIRS,
                minRatio=DEFAULT_MIN_RATIO, minSize=DEFAULT_MIN_SIZE, outFile=None, placedFile=None, fullDir=None, threads=0, device=0,
                context=None):
    """``context``: a context of the caller's - one that has ``anchor_file`` answers each pass in one call, any other is driven
    through anchor_begin / anchor_add_pairs / anchor_finish; None: a context of its own on ``device`` and two passes of
    hicmi_anchor_file."""
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    if outFile is None:
        outFile = os.path.join(v["saveFilesDirectory"], "unplacedSupport.txt")
    with pairtool.refusing(OSError, ValueError):
        pairtool.check_thresholds(window, reach, minPairs, minSize, minRatio)
        names, sizes, orderFile, asm = pairtool.load(v, orderFile)
        first1, n1 = number_blocks(asm, sizes)
        if n1 > MAX_TABLE:
            raise ValueError("%d unplaced scaffolds against %d chromosomes need a table of %d counters, more than the %d a build can "
                             "have; -minSize applies after this pass and cannot make it smaller: take the smallest scaffolds out of "
                             "hicProScaffSizeFile" % (int((first1 >= 0).sum()), len(asm.components), n1, MAX_TABLE))
    n_seq = len(asm.components)
    candidates = np.flatnonzero(first1 >= 0).tolist()
    tables = (asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes)
    filled, B = chromosome_members(asm, sizes)

    zero = np.zeros(6, np.uint64)

    def count(ctx, target, first, n_table):
        """One pass: (stats4, table, counters), the library's blocks checked against this report's."""
        if context is None:
            got = _lib.anchor_file(v["validPairFile"], names, sizes, *tables, target, window, ctx, threads=threads)
        elif hasattr(ctx, "anchor_file"):
            got = ctx.anchor_file(v["validPairFile"], names, sizes, *tables, target, window, threads=threads)
        else:
            got = measure(ctx, v["validPairFile"], names, sizes, asm, target, window, threads)
        stats, got_first, table, counters = got
        if not np.array_equal(got_first, first) or table.shape != (n_table,):
            pairtool.refuse("the library numbers the unplaced scaffolds differently from this report")
        return tuple(stats[:4]), table, counters

    def passes(ctx):
        return both_passes(lambda target, first, n_table: count(ctx, target, first, n_table), asm, sizes, first1, n1, minPairs,
                           minRatio, minSize)

    stats, counters1, counters2, links, chosen, T = (0, 0, 0, 0), zero, zero, {}, {}, {}
    if candidates:
        stats, counters1, counters2, links, chosen, T = pairtool.on_context(context, device, passes)
    else:
        print("UNPLACED: nothing is unplaced: %s names every scaffold that has a base" % orderFile)
    print(pairtool.lines_line("UNPLACED", stats) + "; chromosomes: " + pairtool.counted(COUNTER_COLUMNS, counters1)
          + "; gaps: " + pairtool.counted(COUNTER_COLUMNS, counters2))

    scores, gaps, verdicts, winners = settle_gaps(T, chosen, candidates, reach, minPairs)

    header = ["window=%d" % window, "reach=%d" % reach, "minPairs=%d" % minPairs, "minRatio=%g" % minRatio, "minSize=%d" % minSize]
    header += pairtool.fields(pairtool.STATS_COLUMNS, stats) + pairtool.fields(COUNTER_COLUMNS, counters1.tolist(), "chromosomes_")
    header += pairtool.fields(COUNTER_COLUMNS, counters2.tolist(), "gaps_")
    out = ["#" + "\t".join(header) + "\n", "### Unplaced ###\n", "#" + "\t".join(UNPLACED_COLUMNS) + "\n"]
    for s in candidates:
        best, second, ratio, _verdict = chosen[s]
        a = links[s]
        cols = [names[s], str(int(sizes[s])), str(sum(a))]
        cols += [str(best + 1), str(a[best])] if sum(a) else ["NA", "NA"]
        cols += [str(second + 1), str(a[second])] if sum(a) and second is not None else ["NA", "NA"]
        cols.append(_ratio_text(ratio if sum(a) else None))
        if s in gaps:
            g, o, m, runner_up, verdict = gaps[s]
            cols += ["NA", "NA", "NA"] if verdict == "chromosome_only" else list(pairtool.gap_neighbours(names, filled[best], g)) + ["+-"[o]]
            cols += [str(m), str(runner_up)]
        else:
            cols += ["NA"] * 5
        out.append("\t".join(cols + [verdicts[s]]) + "\n")
    out += ["### Chromosomes ###\n", "#" + "\t".join(CHROMOSOME_COLUMNS) + "\n"]
    for q in range(n_seq):
        out.append("%d\t%d\t%d\t%d\t%d\n" % (q + 1, len(filled[q]), B[q], sum(chosen[s][0] == q for s in T),
                                             sum(key[0] == q for key in winners)))
    insertions = winner_insertions(winners, gaps, filled, names)
    placed_text = None if placedFile is None else placed_order_text(orderFile, insertions)
    pairtool.write_text(outFile, "".join(out), mkdir=True)
    if placedFile is not None:
        pairtool.write_text(placedFile, placed_text, newline="")
    if fullDir is not None:
        pairtool.write_gap_tables(fullDir, "unplaced", names, n_seq, [(s, links[s]) for s in candidates],
                                  [(s, chosen[s][0], filled[chosen[s][0]], scores[s]) for s in sorted(scores)])
    inserted = sorted(winners.values())
    print("UNPLACED: %d unplaced scaffold(s), %d with a chromosome, %d inserted, %d deferred" % (
        len(candidates), len(T), len(inserted), sum(x == "deferred" for x in verdicts.values())))
    return stats, verdicts, {names[s]: (chosen[s][0], gaps[s][0], "+-"[gaps[s][1]]) for s in inserted}


def main(argv=None, context=None):
    parser = argparse.ArgumentParser(description="Counts, on the GPU, the read pairs of validPairFile that link the scaffolds an order "
                                                 "file leaves out to its chromosomes and to the ends of their scaffolds, and "
                                                 "reports where each of them belongs.")
    with pairtool.common_arguments(parser):
        parser.add_argument("-window", help="End zone of a placed scaffold in bp (default %d)" % DEFAULT_WINDOW, type=int,
                            default=DEFAULT_WINDOW)
        parser.add_argument("-reach", help="Scaffolds on either side of a gap that score it, 1 .. %d (default %d)" % (MAX_REACH, DEFAULT_REACH),
                            type=int, default=DEFAULT_REACH)
        parser.add_argument("-minPairs", help="Links below which neither a chromosome nor a gap is chosen (default %d)" % DEFAULT_MIN_PAIRS,
                            type=int, default=DEFAULT_MIN_PAIRS)
        parser.add_argument("-minRatio", help="Link density of the best chromosome over the second best below which none is chosen "
                                              "(default %g)" % DEFAULT_MIN_RATIO, type=float, default=DEFAULT_MIN_RATIO)
        parser.add_argument("-minSize", help="Scaffolds below this size in bp get no chromosome (default %d)" % DEFAULT_MIN_SIZE, type=int,
                            default=DEFAULT_MIN_SIZE)
        parser.add_argument("-out", help="Report (default: saveFilesDirectory/unplacedSupport.txt)", type=str, default=None)
        parser.add_argument("-placed", help="Write the order file again with one placed scaffold inserted per gap", type=str, default=None)
        parser.add_argument("-full", help="Write unplaced.chromosomes.tsv and unplaced.gaps.tsv into this directory", type=str, default=None)
    args = parser.parse_args(argv)
    return runPipeline(args.config, args.order, args.window, args.reach, args.minPairs, args.minRatio, args.minSize, args.out, args.placed,
                       args.full, threads=args.threads, device=args.device, context=context)


if __name__ == "__main__":
    main()

