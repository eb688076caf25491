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
import sys

import numpy as np

from . import _lib
from . import placeUnplaced as place
from .assembledMap import DEFAULT_GAP, build_assembly, read_order_file
from .buildMap import STATS_COLUMNS, check_valid_pair_file
from .hostio import paused_gc, read_scaffold_sizes

DEFAULT_WINDOW, DEFAULT_REACH, DEFAULT_MIN_PAIRS, DEFAULT_MIN_RATIO = 50000, 2, 4, 2.0
MAX_REACH = 64
MAX_TABLE = 1 << 27
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


def moved_order_text(orderFile, moves):
    """The order file again with the line of every scaffold of ``moves`` - {name: (where, orientation)} - taken out and put
    back before the line of the scaffold ``where``, or after it when ``where`` is (name, None), its sign set to
    ``orientation``.  Every other byte of every line is kept; a file without a final newline stays one."""
    with open(orderFile, newline="") as fh:
        lines = list(fh)

    def name_of(k):
        body = lines[k].rstrip("\r\n")
        return body.split("\t")[0] if k and body and body[0] != "#" else None

    taken = {}
    for k in range(len(lines)):
        name = name_of(k)
        if name in moves:
            body = lines[k].rstrip("\r\n")
            cols = body.split("\t")
            cols[1] = moves[name][1]
            taken[name] = "\t".join(cols) + lines[k][len(body):]
    before = {where: name for name, (where, _o) in moves.items() if not isinstance(where, tuple)}
    after = {where[0]: name for name, (where, _o) in moves.items() if isinstance(where, tuple)}
    out = []
    for k, line in enumerate(lines):
        name = name_of(k)
        if name in taken:
            continue
        if name is not None and name in before:
            out.append(taken[before[name]])
        out.append(line)
        if name is not None and name in after:
            out.append(taken[after[name]])
    # the one line without an ending was the last one: inside the file it takes its neighbour's, and the new last line has none
    final = bool(lines) and lines[-1].endswith(("\n", "\r"))
    for k, line in enumerate(out):
        body = line.rstrip("\r\n")
        if k < len(out) - 1 and body == line:
            nxt = out[k + 1]
            out[k] = body + (nxt[len(nxt.rstrip("\r\n")):] or "\n")
        elif k == len(out) - 1 and not final:
            out[k] = body
    return "".join(out)


def check_arguments(window, reach, minPairs, minRatio):
    if window < 1:
        raise ValueError("the window %d is below 1" % window)
    if not 1 <= reach <= MAX_REACH:
        raise ValueError("the reach %d is outside 1 .. %d" % (reach, MAX_REACH))
    if minPairs < 0:
        raise ValueError("minPairs %d is negative" % minPairs)
    if not minRatio >= 1:
        raise ValueError("minRatio %g is below 1" % minRatio)


def runPipeline(configFile, orderFile=None, window=DEFAULT_WINDOW, reach=DEFAULT_REACH, minPairs=DEFAULT_MIN_PAIRS,
                minRatio=DEFAULT_MIN_RATIO, outFile=None, movedFile=None, fullDir=None, threads=0, device=0, context=None):
    """``context``: a context of the caller's that has ``pairs_file``, ``seats_resident`` and ``pairs_drop``; None: a context
    of its own on ``device``.  Either way the file is loaded into the resident pair store, counted in one call and the store
    dropped.  Returns (stats4, verdicts {name: verdict}, moves {name: (chromosome, gap, orientation)})."""
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    if outFile is None:
        outFile = os.path.join(v["saveFilesDirectory"], "seatSupport.txt")
    try:
        check_arguments(window, reach, minPairs, minRatio)
        check_valid_pair_file(v["validPairFile"])
        names, sizes = read_scaffold_sizes(v["hicProScaffSizeFile"])
        if not names:
            raise ValueError("hicProScaffSizeFile %s lists no scaffold" % v["hicProScaffSizeFile"])
        if orderFile is None:
            orderFile = v["finalOrderingsFile"] if os.path.isfile(v["finalOrderingsFile"]) else v["chromosomeOrderFile"]
        if not os.path.isfile(orderFile):
            raise ValueError("order file %r does not exist" % orderFile)
        asm = build_assembly(read_order_file(orderFile), names, sizes, DEFAULT_GAP, chromosomes_only=True)
        n_placed = _lib.ends_placed_count(sizes, asm.lift_seq)
        if n_placed < 1:
            raise ValueError("no scaffold of %s has a base" % orderFile)
        first, n_table = number_blocks(asm, sizes)
        if n_table > MAX_TABLE:
            raise ValueError("%d placed scaffolds in %d chromosomes need a table of %d counters, more than the %d a call can have"
                             % (n_placed, len(asm.components), n_table, MAX_TABLE))
    except (OSError, ValueError) as exc:
        sys.exit("ERROR... %s. Exiting..." % exc)
    n_seq = len(asm.components)

    def count(ctx):
        stats = tuple(ctx.pairs_file(v["validPairFile"], names, sizes, threads=threads)[:4])
        try:
            return (stats,) + tuple(ctx.seats_resident(sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, window))
        finally:
            ctx.pairs_drop()

    with paused_gc():
        try:
            if context is None:
                with _lib.Context(device) as ctx:
                    stats, got_first, table, counters = count(ctx)
            else:
                stats, got_first, table, counters = count(context)
        except _lib.HicmiError as exc:
            sys.exit("ERROR... %s. Exiting..." % exc)
    if not np.array_equal(got_first, first) or table.shape != (n_table,):
        sys.exit("ERROR... the library numbers the placed scaffolds differently from this report. Exiting...")
    print("SEATS: lines %d, pairs used %d, unknown scaffold %d, out of range %d" % stats
          + ", " + ", ".join("%s %d" % kv for kv in zip(COUNTER_COLUMNS, counters.tolist())))

    calls = seat_calls(asm, sizes, first, table, reach, minPairs, minRatio)
    moves = chosen_moves(asm, sizes, calls)
    filled, _B = place.chromosome_members(asm, sizes)
    header = ["window=%d" % window, "reach=%d" % reach, "minPairs=%d" % minPairs, "minRatio=%g" % minRatio]
    header += ["%s=%d" % kv for kv in zip(STATS_COLUMNS, stats)] + ["%s=%d" % kv for kv in zip(COUNTER_COLUMNS, counters.tolist())]
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
                if gap_verdict == "chromosome_only":
                    cols += ["NA", "NA", "NA"]
                else:
                    cols += [names[others[g - 1]] if g else "start", names[others[g]] if g < len(others) else "end", "+-"[o]]
                cols += [str(m), str(runner_up), str(call["gain"])]
            else:
                cols += ["NA"] * 7
            out.append("\t".join(cols + [call["verdict"]]) + "\n")
    moved_text = None if movedFile is None else moved_order_text(orderFile, move_targets(asm, sizes, calls, moves, names))
    os.makedirs(os.path.dirname(os.path.abspath(outFile)), exist_ok=True)
    with open(outFile, "w") as fh:
        fh.write("".join(out))
    if movedFile is not None:
        with open(movedFile, "w", newline="") as fh:
            fh.write(moved_text)
    if fullDir is not None:
        os.makedirs(fullDir, exist_ok=True)
        with open(os.path.join(fullDir, "seats.chromosomes.tsv"), "w") as fh:
            fh.write("#scaffold\t" + "\t".join("Chr_%d" % (q + 1) for q in range(n_seq)) + "\n")
            for s in sorted(s for s in calls if "a" in calls[s]):
                fh.write(names[s] + "\t" + "\t".join(str(x) for x in calls[s]["a"]) + "\n")
        with open(os.path.join(fullDir, "seats.gaps.tsv"), "w") as fh:
            fh.write("#scaffold\tchromosome\tgap\tleft\tright\torientation\tscore\n")
            for s in sorted(s for s in calls if "scores" in calls[s]):
                q = calls[s]["q"]
                others = [t for t in filled[q] if t != s]
                for g, both in enumerate(calls[s]["scores"]):
                    for o, x in enumerate(both):
                        fh.write("%s\t%d\t%d\t%s\t%s\t%s\t%d\n" % (names[s], q + 1, g, names[others[g - 1]] if g else "start",
                                                                   names[others[g]] if g < len(others) else "end", "+-"[o], x))
    tally = {w: sum(x == w for x in verdicts.values()) for w in ("move", "flip", "elsewhere", "open")}
    print("SEATS: %d scaffold(s) to move, %d to flip, %d elsewhere, %d open; %d move(s) chosen" % (
        tally["move"], tally["flip"], tally["elsewhere"], tally["open"], len(moves)))
    return stats, verdicts, {names[s]: (q, calls[s]["gap"][0], "+-"[calls[s]["gap"][1]]) for q, s in moves.items()}


def main(argv=None, context=None):
    parser = argparse.ArgumentParser(description="Counts, on the GPU, for every scaffold of an order file the read pairs of "
                                                 "validPairFile that link it to the chromosomes and to the ends of the scaffolds "
                                                 "of its own, and reports whether it lies where they place it.")
    parser.add_argument("-config", help="Full file path to the config file", required=True, type=str)
    parser.add_argument("-order", help="Order file (default: finalOrderingsFile when it exists, else chromosomeOrderFile)",
                        type=str, default=None)
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
    parser.add_argument("-threads", help="Host threads of the parser (default 0: all)", type=int, default=0)
    parser.add_argument("-device", help="GPU index (default 0)", type=int, default=0)
    args = parser.parse_args(argv)
    return runPipeline(args.config, args.order, args.window, args.reach, args.minPairs, args.minRatio, args.out, args.moved, args.full,
                       threads=args.threads, device=args.device, context=context)


if __name__ == "__main__":
    main()
