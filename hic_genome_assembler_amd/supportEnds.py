"""End support: the read pairs that link the ends of neighbouring scaffolds of an ordering, on the device (DESIGN.md
section 9p).

Every orientation the other reports give is read from the binned contact map, which says nothing about a scaffold of one
bin; supportSpans counts how many pairs bridge a junction, not which ends they join.  This one reads ``validPairFile``
itself: every scaffold of the order file has a left and a right end zone of ``-window`` bp as it lies in its chromosome (a
scaffold of up to two windows is cut in halves), and for every two scaffolds at most ``-reach`` places apart the read pairs
between their zones are counted in the four combinations left-left, left-right, right-left and right-right.  A scaffold
that lies the right way round is linked to its neighbours through the ends that face them; one that lies the wrong way
round through the far ones.

    python -m hic_genome_assembler_amd.supportEnds -config my_config.txt [-order FILE] [-window 50000] [-reach 2] [-minPairs 4] \\
           [-out FILE] [-flipped FILE] [-full DIR] [-threads 0] [-device 0]

Per scaffold ``as_lies`` is the number of links its ends have with the facing ends of its neighbours, ``flipped`` the number
they would have if the scaffold alone were turned round; the verdict is ``supported``, ``flip``, ``open`` (a tie, or fewer
than ``-minPairs`` links in all) or ``NA`` (alone in its chromosome).  Per junction the four combinations are listed and the
verdict names the strict maximum: ``held``, ``flip_left``, ``flip_right``, ``flip_both`` or ``open``.  Every verdict is
judged on the order file as it lies, not one after the other.  The scaffolds the order file does not name take no part:
their pairs are counted as ``unlifted``.  There is no restriction-site normalisation; the two zones of a scaffold are
equally long to within one base.  The defaults of ``-window``, ``-reach`` and ``-minPairs`` are choices, not tuned values.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import _lib, pairtool
from .pairtool import DEFAULT_MIN_PAIRS, DEFAULT_REACH, DEFAULT_WINDOW, MAX_REACH, MAX_TABLE, flipped_order_text  # noqa: F401

COUNTER_COLUMNS = ("linked", "middle", "same", "too_far", "trans", "unlifted")
SCAFFOLD_COLUMNS = ("scaffold", "orientation", "size", "left_zone", "right_zone", "as_lies", "flipped", "verdict")
JUNCTION_COLUMNS = ("chromosome", "left", "right", "facing", "left_flipped", "right_flipped", "both_flipped", "verdict")
LINK_COLUMNS = ("scaffold", "d", "neighbour", "left_left", "left_right", "right_left", "right_right")
JUNCTION_VERDICTS = ("held", "flip_left", "flip_right", "flip_both")
LL, LR, RL, RR = 0, 1, 2, 3                    # zone at the lower rank x zone at the higher rank


def number_ranks(asm, sizes):
    """(rank int32[S], seq_first int64[n_seq + 1]) of DESIGN.md 9p from the components of the assembly: the placed scaffolds
    of size > 0 in sequence order."""
    rank = np.full(len(sizes), -1, np.int32)
    seq_first = np.zeros(len(asm.components) + 1, np.int64)
    n = 0
    for q, comps in enumerate(asm.components):
        for s, _off, _orientation in comps:
            if sizes[s] > 0:
                rank[s] = n
                n += 1
        seq_first[q + 1] = n
    return rank, seq_first


def zone_sizes(L, window):
    """(left zone, right zone) of a scaffold of L bases as it lies, in bases."""
    return min(window, L - L // 2), min(window, L // 2)


def scaffold_figures(T, i, q0, q1):
    """(as_lies, flipped) of the scaffold of rank i in the sequence with the ranks [q0, q1), from the table
    T[rank, d - 1, zone x zone]."""
    as_lies = flipped = 0
    for d in range(1, T.shape[1] + 1):
        if i + d < q1:
            as_lies += int(T[i, d - 1, RL])
            flipped += int(T[i, d - 1, LL])
        if i - d >= q0:
            as_lies += int(T[i - d, d - 1, RL])
            flipped += int(T[i - d, d - 1, RR])
    return as_lies, flipped


def scaffold_verdict(as_lies, flipped, alone, minPairs):
    if alone:
        return "NA"
    if as_lies == flipped or as_lies + flipped < minPairs:
        return "open"
    return "supported" if as_lies > flipped else "flip"


def scaffold_calls(asm, sizes, rank, seq_first, T, minPairs):
    """{scaffold: (as_lies, flipped, verdict)} of every scaffold of the assembly that has a base: the decision the report
    writes down and polishOrder acts on."""
    calls = {}
    for q, comps in enumerate(asm.components):
        q0, q1 = int(seq_first[q]), int(seq_first[q + 1])
        for s, _off, _orientation in comps:
            if rank[s] >= 0:
                as_lies, flipped = scaffold_figures(T, int(rank[s]), q0, q1)
                calls[s] = (as_lies, flipped, scaffold_verdict(as_lies, flipped, q1 - q0 == 1, minPairs))
    return calls


def junction_figures(T, i):
    """(facing, left_flipped, right_flipped, both_flipped) of the junction between the ranks i and i + 1."""
    return [int(T[i, 0, k]) for k in (RL, LL, RR, LR)]


def junction_verdict(figures, minPairs):
    best = max(figures)
    if sum(figures) < minPairs or figures.count(best) != 1:
        return "open"
    return JUNCTION_VERDICTS[figures.index(best)]


def measure(ctx, pairFile, names, sizes, asm, window, reach, threads):
    """(stats4, rank, table, counters) through the array calls of a context the caller owns: the file is parsed on the host
    in chunks (hicmi_parse_valid_pairs) and counted chunk by chunk."""
    rank = ctx.ends_begin(sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, window, reach)
    stats = pairtool.parse_in_chunks(pairFile, names, sizes, threads, ctx.ends_add_pairs)
    table, counters = ctx.ends_finish()
    return stats, rank, table, counters


def runPipeline(configFile, orderFile=None, window=DEFAULT_WINDOW, reach=DEFAULT_REACH, minPairs=DEFAULT_MIN_PAIRS, outFile=None,
                flippedFile=None, fullDir=None, threads=0, device=0, context=None):
    """``context``: a context of the caller's - one that has ``ends_file`` answers in one call, any other is driven through
    ends_begin / ends_add_pairs / ends_finish; None: a context of its own on ``device`` and one pass of hicmi_ends_file."""
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    if outFile is None:
        outFile = os.path.join(v["saveFilesDirectory"], "endSupport.txt")
    with pairtool.refusing(OSError, ValueError):
        pairtool.check_thresholds(window=window, reach=reach, minPairs=minPairs)
        names, sizes, orderFile, asm = pairtool.load(v, orderFile)
        n_placed = _lib.ends_placed_count(sizes, asm.lift_seq)
        if n_placed * reach * 4 > MAX_TABLE:
            raise ValueError("reach %d over %d placed scaffolds needs a table of %d counters, more than the %d a build can have"
                             % (reach, n_placed, n_placed * reach * 4, MAX_TABLE))
        if n_placed < 1:
            raise ValueError("no scaffold of %s has a base" % orderFile)
    rank, seq_first = number_ranks(asm, sizes)
    tables = (asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes)

    def count(ctx):
        if context is None:
            return _lib.ends_file(v["validPairFile"], names, sizes, *tables, window, reach, ctx, threads=threads)
        if hasattr(ctx, "ends_file"):
            return ctx.ends_file(v["validPairFile"], names, sizes, *tables, window, reach, threads=threads)
        return measure(ctx, v["validPairFile"], names, sizes, asm, window, reach, threads)

    stats, got_rank, T, counters = pairtool.on_context(context, device, count)
    if not np.array_equal(got_rank, rank) or T.shape != (n_placed, reach, 4):
        pairtool.refuse("the library ranks the scaffolds differently from this report")
    stats = tuple(stats[:4])
    print(pairtool.lines_line("ENDS", stats) + ", " + pairtool.counted(COUNTER_COLUMNS, counters))

    header = ["window=%d" % window, "reach=%d" % reach, "minPairs=%d" % minPairs]
    header += pairtool.fields(pairtool.STATS_COLUMNS, stats) + pairtool.fields(COUNTER_COLUMNS, counters.tolist())
    out = ["#" + "\t".join(header) + "\n", "#" + "\t".join(SCAFFOLD_COLUMNS) + "\n"]
    flips, junctions, verdicts = set(), [], {}
    calls = scaffold_calls(asm, sizes, rank, seq_first, T, minPairs)
    for q, comps in enumerate(asm.components):
        out.append("### Chromosome grouping %d ###\n" % (q + 1))
        for s, _off, orientation in comps:
            L = int(sizes[s])
            if rank[s] < 0:                                                    # a scaffold without a base has no ends
                cols = ["0", "0", "0", "0", "NA"]
            else:
                as_lies, flipped, verdict = calls[s]
                cols = [str(x) for x in zone_sizes(L, window) + (as_lies, flipped)] + [verdict]
            verdicts[names[s]] = cols[-1]
            if cols[-1] == "flip":
                flips.add(names[s])
            out.append("\t".join([names[s], orientation, str(L)] + cols) + "\n")
        filled = [s for s, _off, _o in comps if sizes[s] > 0]
        for left, right in zip(filled, filled[1:]):
            figures = junction_figures(T, int(rank[left]))
            junctions.append("\t".join([str(q + 1), names[left], names[right]] + [str(x) for x in figures]
                                       + [junction_verdict(figures, minPairs)]) + "\n")
    out += ["### Junctions ###\n", "#" + "\t".join(JUNCTION_COLUMNS) + "\n"] + junctions
    flipped_text = None if flippedFile is None else flipped_order_text(orderFile, flips)
    pairtool.write_text(outFile, "".join(out), mkdir=True)
    if flippedFile is not None:
        pairtool.write_text(flippedFile, flipped_text, newline="")
    if fullDir is not None:
        links = ["#" + "\t".join(LINK_COLUMNS) + "\n"]
        for comps in asm.components:
            filled = [s for s, _off, _o in comps if sizes[s] > 0]
            for k, s in enumerate(filled):
                for d in range(1, min(reach, len(filled) - 1 - k) + 1):
                    links.append("%s\t%d\t%s\t%d\t%d\t%d\t%d\n" % ((names[s], d, names[filled[k + d]]) + tuple(int(x) for x in T[rank[s], d - 1])))
        pairtool.write_text(os.path.join(fullDir, "ends.links.tsv"), "".join(links), mkdir=True)
    n_open = sum(x == "open" for x in verdicts.values())
    print("ENDS: %d scaffold(s) to flip, %d open, %d of %d junction(s) not held" % (
        len(flips), n_open, sum(not j.endswith("\theld\n") for j in junctions), len(junctions)))
    return stats, T, counters, sorted(flips)


def main(argv=None, context=None):
    parser = argparse.ArgumentParser(description="Counts, on the GPU, the read pairs of validPairFile that link the end zones of "
                                                 "neighbouring scaffolds of an ordering, and reports which scaffolds lie the wrong "
                                                 "way round.")
    with pairtool.common_arguments(parser):
        parser.add_argument("-window", help="End zone in bp (default %d)" % DEFAULT_WINDOW, type=int, default=DEFAULT_WINDOW)
        parser.add_argument("-reach", help="Places two scaffolds may lie apart, 1 .. %d (default %d)" % (MAX_REACH, DEFAULT_REACH),
                            type=int, default=DEFAULT_REACH)
        parser.add_argument("-minPairs", help="Links below which a verdict stays open (default %d)" % DEFAULT_MIN_PAIRS, type=int,
                            default=DEFAULT_MIN_PAIRS)
        parser.add_argument("-out", help="Report (default: saveFilesDirectory/endSupport.txt)", type=str, default=None)
        parser.add_argument("-flipped", help="Write the order file again with the sign of every scaffold called flip changed", type=str,
                            default=None)
        parser.add_argument("-full", help="Write ends.links.tsv, the four counts of every entry inside a chromosome, into this directory",
                            type=str, default=None)
    args = parser.parse_args(argv)
    return runPipeline(args.config, args.order, args.window, args.reach, args.minPairs, args.out, args.flipped, args.full,
                       threads=args.threads, device=args.device, context=context)


if __name__ == "__main__":
    main()
