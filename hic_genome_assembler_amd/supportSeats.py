"""Seat support: every placed scaffold of an ordering taken out and re-placed from its read pairs, on the device (DESIGN.md
section 9s).

supportEnds turns a scaffold round and placeUnplaced inserts one that is missing; neither questions where a placed scaffold
lies.  The seat of a scaffold is its chromosome, gap and orientation.  This tool loads ``validPairFile`` into the resident
pair store of a context and counts, in one kernel launch over the store, for every placed scaffold what placeUnplaced would
count if that scaffold alone were left out of the order file: its links with every chromosome, and the links of its two
halves with the end zones of ``-window`` bp of the scaffolds of its own chromosome.  The decisions are placeUnplaced's own
functions: the chromosome it is linked to most densely, then the best gap and orientation of its chromosome.

    python -m hic_genome_assembler_amd.supportSeats -config my_config.txt [-order FILE] [-window 50000] [-reach 2] [-minPairs 4] \\
           [-minRatio 2] [-out FILE] [-moved FILE] [-full DIR] [-threads 0] [-device 0]

Verdicts, checked in this order: ``NA`` (no base), ``no_links``, ``elsewhere`` (another chromosome stands out; reported,
never applied), ``alone`` (no other scaffold with a base in its chromosome), ``open`` (no gap stands out), ``move`` (the best
gap is not the one it lies in), ``orientation_open`` (its own gap, both orientations score the same), ``flip`` (its own gap,
the other way round) and ``supported``.  ``gain`` is the score of the best seat less the score of the seat it has.
``-moved`` writes the order file again with one move per chromosome applied: the ``move`` of the highest gain, then of the
lowest rank.  The scaffolds the order file does not name take no part.  There is no restriction-site normalisation.  The
defaults are choices, not tuned values.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import _lib, pairtool
from . import placeUnplaced as place
from .pairtool import (DEFAULT_MIN_PAIRS, DEFAULT_MIN_RATIO, DEFAULT_REACH, DEFAULT_WINDOW, MAX_REACH, MAX_TABLE,  # noqa: F401
                       moved_order_text)

COUNTER_COLUMNS = ("seated", "middle", "trans", "same", "unlifted")
SEAT_COLUMNS = ("scaffold", "orientation", "size", "links", "chrom_links", "best_chromosome", "ratio", "home_score", "left", "right",
                "best_orientation", "score", "runner_up", "gain", "verdict")


def number_blocks(asm, sizes):
    """(first int64[S], n_table) of DESIGN.md 9s from the components of the assembly: the placed scaffolds with a base in
    size-file order, each with a block of one counter per sequence and four per scaffold with a base of its own sequence."""
    filled = [sum(1 for s, _off, _o in comps if sizes[s] > 0) for comps in asm.components]
    first = np.full(len(sizes), -1, np.int64)
    n = 0
    for s in range(len(sizes)):
        if asm.lift_seq[s] >= 0 and sizes[s] > 0:
            first[s] = n
            n += len(asm.components) + 4 * filled[asm.lift_seq[s]]
    return first, n


def table_size(n_seq, filled_counts):
    """Counters of the table of an assembly with ``filled_counts[q]`` scaffolds with a base in sequence q."""
    return sum(S * (n_seq + 4 * S) for S in filled_counts)


def seat_calls(asm, sizes, first, table, reach, minPairs, minRatio):
    """{scaffold: dict} for every scaffold of the assembly: ``verdict`` and, with a base, ``q``, ``k`` (its local rank),
    ``o`` (0: +, 1: -), ``a`` (links per chromosome), ``chosen`` (choose_chromosome without it), and with company in its
    chromosome ``scores`` (gap_scores without it), ``gap`` (choose_gap), ``home_score`` and ``gain``.  The decision the report
    writes down and polishOrder acts on."""
    n_seq = len(asm.components)
    filled, B = place.chromosome_members(asm, sizes)
    calls = {}
    for q, comps in enumerate(asm.components):
        S = len(filled[q])
        for s, _off, orientation in comps:
            if first[s] < 0:
                calls[s] = {"verdict": "NA"}
                continue
            at = int(first[s])
            a = [int(x) for x in table[at:at + n_seq]]
            k = filled[q].index(s)
            without = list(B)
            without[q] -= int(sizes[s])
            chosen = place.choose_chromosome(a, without, int(sizes[s]), minPairs, minRatio, 0)
            call = {"q": q, "k": k, "o": int(orientation == "-"), "a": a, "chosen": chosen}
            if S > 1:
                T = np.delete(table[at + n_seq:at + n_seq + 4 * S].reshape(S, 2, 2), k, axis=0)
                call["scores"] = place.gap_scores(T, reach)
                call["gap"] = place.choose_gap(call["scores"], minPairs)
                call["home_score"] = call["scores"][k][call["o"]]
                call["gain"] = call["gap"][2] - call["home_score"]
            if sum(a) == 0:
                verdict = "no_links"
            elif chosen[3] is None and chosen[0] != q:
                verdict = "elsewhere"
            elif S == 1:
                verdict = "alone"
            elif call["gap"][4] == "chromosome_only":
                verdict = "open"
            elif call["gap"][0] != k:
                verdict = "move"
            elif call["gap"][4] == "orientation_open":
                verdict = "orientation_open"
            else:
                verdict = "flip" if call["gap"][1] != call["o"] else "supported"
            call["verdict"] = verdict
            calls[s] = call
    return calls


def chosen_moves(asm, sizes, calls):
    """{chromosome: scaffold}: per chromosome the scaffold called ``move`` of the highest gain, then of the lowest rank."""
    moves = {}
    filled, _B = place.chromosome_members(asm, sizes)
    for q, members in enumerate(filled):
        wanting = [s for s in members if calls[s]["verdict"] == "move"]
        if wanting:
            moves[q] = min(wanting, key=lambda s: (-calls[s]["gain"], calls[s]["k"]))
    return moves


def move_targets(asm, sizes, calls, moves, names):
    """The moves as ``moved_order_text`` takes them: {name: (where, orientation)}, ``where`` the name of the scaffold after
    the new gap or (name of the chromosome's last other scaffold, None) for the last gap."""
    filled, _B = place.chromosome_members(asm, sizes)
    out = {}
    for q, s in moves.items():
        others = [t for t in filled[q] if t != s]
        g, o = calls[s]["gap"][:2]
        out[names[s]] = (names[others[g]] if g < len(others) else (names[others[-1]], None), "+-"[o])
    return out


def runPipeline(configFile, orderFile=None, window=DEFAULT_WINDOW, reach=DEFAULT_REACH, minPairs=DEFAULT_MIN_PAIRS,
                minRatio=DEFAULT_MIN_RATIO, outFile=None, movedFile=None, fullDir=None, threads=0, device=0, context=None):
    """``context``: a context of the caller's that has ``pairs_file``, ``seats_resident`` and ``pairs_drop``; None: a context
    of its own on ``device``.  Either way the file is loaded into the resident pair store, counted in one call and the store
    dropped.  Returns (stats4, verdicts {name: verdict}, moves {name: (chromosome, gap, orientation)})."""
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    if outFile is None:
        outFile = os.path.join(v["saveFilesDirectory"], "seatSupport.txt")
    with pairtool.refusing(OSError, ValueError):
        pairtool.check_thresholds(window=window, reach=reach, minPairs=minPairs, minRatio=minRatio)
        names, sizes, orderFile, asm = pairtool.load(v, orderFile)
        n_placed = _lib.ends_placed_count(sizes, asm.lift_seq)
        if n_placed < 1:
            raise ValueError("no scaffold of %s has a base" % orderFile)
        first, n_table = number_blocks(asm, sizes)
        if n_table > MAX_TABLE:
            raise ValueError("%d placed scaffolds in %d chromosomes need a table of %d counters, more than the %d a call can have"
                             % (n_placed, len(asm.components), n_table, MAX_TABLE))
    n_seq = len(asm.components)

    def count(ctx):
        stats = tuple(ctx.pairs_file(v["validPairFile"], names, sizes, threads=threads)[:4])
        try:
            return (stats,) + tuple(ctx.seats_resident(sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, window))
        finally:
            ctx.pairs_drop()

    stats, got_first, table, counters = pairtool.on_context(context, device, count)
    if not np.array_equal(got_first, first) or table.shape != (n_table,):
        pairtool.refuse("the library numbers the placed scaffolds differently from this report")
    print(pairtool.lines_line("SEATS", stats) + ", " + pairtool.counted(COUNTER_COLUMNS, counters))

    calls = seat_calls(asm, sizes, first, table, reach, minPairs, minRatio)
    moves = chosen_moves(asm, sizes, calls)
    filled, _B = place.chromosome_members(asm, sizes)
    header = ["window=%d" % window, "reach=%d" % reach, "minPairs=%d" % minPairs, "minRatio=%g" % minRatio]
    header += pairtool.fields(pairtool.STATS_COLUMNS, stats) + pairtool.fields(COUNTER_COLUMNS, counters.tolist())
    out = ["#" + "\t".join(header) + "\n", "#" + "\t".join(SEAT_COLUMNS) + "\n"]
    verdicts = {}
    for q, comps in enumerate(asm.components):
        out.append("### Chromosome grouping %d ###\n" % (q + 1))
        for s, _off, orientation in comps:
            call = calls[s]
            verdicts[names[s]] = call["verdict"]
            cols = [names[s], orientation, str(int(sizes[s]))]
            if call["verdict"] == "NA":
                out.append("\t".join(cols + ["NA"] * 11 + ["NA"]) + "\n")
                continue
            a, (best, _second, ratio, _verdict) = call["a"], call["chosen"]
            links = sum(a)
            cols += [str(links), str(a[q]), str(best + 1) if links else "NA", place._ratio_text(ratio if links else None)]
            if "gap" in call:
                g, o, m, runner_up, gap_verdict = call["gap"]
                others = [t for t in filled[q] if t != s]
                cols.append(str(call["home_score"]))
                cols += ["NA", "NA", "NA"] if gap_verdict == "chromosome_only" else list(pairtool.gap_neighbours(names, others, g)) + ["+-"[o]]
                cols += [str(m), str(runner_up), str(call["gain"])]
            else:
                cols += ["NA"] * 7
            out.append("\t".join(cols + [call["verdict"]]) + "\n")
    moved_text = None if movedFile is None else moved_order_text(orderFile, move_targets(asm, sizes, calls, moves, names))
    pairtool.write_text(outFile, "".join(out), mkdir=True)
    if movedFile is not None:
        pairtool.write_text(movedFile, moved_text, newline="")
    if fullDir is not None:
        pairtool.write_gap_tables(fullDir, "seats", names, n_seq, [(s, calls[s]["a"]) for s in sorted(calls) if "a" in calls[s]],
                                  [(s, calls[s]["q"], [t for t in filled[calls[s]["q"]] if t != s], calls[s]["scores"])
                                   for s in sorted(calls) if "scores" in calls[s]])
    tally = {w: sum(x == w for x in verdicts.values()) for w in ("move", "flip", "elsewhere", "open")}
    print("SEATS: %d scaffold(s) to move, %d to flip, %d elsewhere, %d open; %d move(s) chosen" % (
        tally["move"], tally["flip"], tally["elsewhere"], tally["open"], len(moves)))
    return stats, verdicts, {names[s]: (q, calls[s]["gap"][0], "+-"[calls[s]["gap"][1]]) for q, s in moves.items()}


def main(argv=None, context=None):
    parser = argparse.ArgumentParser(description="Counts, on the GPU, for every scaffold of an order file the read pairs of "
                                                 "validPairFile that link it to the chromosomes and to the ends of the scaffolds "
                                                 "of its own, and reports whether it lies where they place it.")
    with pairtool.common_arguments(parser):
        parser.add_argument("-window", help="End zone of a scaffold in bp (default %d)" % DEFAULT_WINDOW, type=int, default=DEFAULT_WINDOW)
        parser.add_argument("-reach", help="Scaffolds on either side of a gap that score it, 1 .. %d (default %d)" % (MAX_REACH, DEFAULT_REACH),
                            type=int, default=DEFAULT_REACH)
        parser.add_argument("-minPairs", help="Links below which neither a chromosome nor a gap is chosen (default %d)" % DEFAULT_MIN_PAIRS,
                            type=int, default=DEFAULT_MIN_PAIRS)
        parser.add_argument("-minRatio", help="Link density of the best chromosome over the second best below which none is chosen "
                                              "(default %g)" % DEFAULT_MIN_RATIO, type=float, default=DEFAULT_MIN_RATIO)
        parser.add_argument("-out", help="Report (default: saveFilesDirectory/seatSupport.txt)", type=str, default=None)
        parser.add_argument("-moved", help="Write the order file again with one move per chromosome applied", type=str, default=None)
        parser.add_argument("-full", help="Write seats.chromosomes.tsv and seats.gaps.tsv into this directory", type=str, default=None)
    args = parser.parse_args(argv)
    return runPipeline(args.config, args.order, args.window, args.reach, args.minPairs, args.minRatio, args.out, args.moved, args.full,
                       threads=args.threads, device=args.device, context=context)


if __name__ == "__main__":
    main()
