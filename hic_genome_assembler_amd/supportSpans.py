"""Span support: the read pairs that span every cut of every scaffold and every junction of an ordering, on the device
(DESIGN.md section 9n).

The reports that read the binned contact map cannot see below one bin.  This one reads ``validPairFile`` itself: the
assembly (``assembledMap.build_assembly``) is cut into cells of ``-step`` bp, scaffold by scaffold from the left end as the
scaffold lies in its chromosome, and for every cell boundary the read pairs with one end on each side are counted - the
spanning depth, or physical coverage.  A misjoin inside a scaffold shows as a dip of the depth against its flanks; a
junction that is right shows none, a wrong one is bridged only by the trans background.

    python -m hic_genome_assembler_amd.supportSpans -config my_config.txt [-order FILE | -scaffolds] [-gap 100] [-step 10000] \\
           [-maxSpan 0] [-flank 8] [-minRatio 0.2] [-out FILE] [-cuts FILE] [-full DIR] [-threads 0] [-device 0]

Per scaffold the interior boundary of lowest ratio depth x flank / min(left flank sum, right flank sum) is reported with the
base of the scaffold's own + coordinate after which it falls, and ``suspect`` when the ratio is below ``-minRatio``; per
junction of two consecutive scaffolds the same ratio at the junction, ``weak`` when it is below.  ``NA``: the flanks do
not fit into the chromosome or hold no pair.  ``-step``, ``-flank`` and ``-minRatio`` defaults are choices, not tuned values.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

from . import _lib, pairtool
from .assembledMap import DEFAULT_GAP, build_assembly

DEFAULT_STEP, DEFAULT_FLANK, DEFAULT_MIN_RATIO = 10000, 8, 0.2
MAX_FLANK = 4096
MAX_CELLS = 1 << 27
COUNTER_COLUMNS = ("marked", "one_cell", "beyond_max_span", "trans", "unlifted")
SCAFFOLD_COLUMNS = ("scaffold", "orientation", "size", "cells", "cut_after", "depth", "flank_depth", "ratio", "verdict")
JUNCTION_COLUMNS = ("chromosome", "left", "right", "depth", "flank_depth", "ratio", "verdict")


def identity_assembly(names, sizes):
    """Every scaffold a + sequence of its own (``-scaffolds``)."""
    return build_assembly([], names, sizes, 0)


def number_cells(asm, sizes, step):
    """(cell_first int64[S], seq_first int64[n_seq + 1]) of DESIGN.md 9n from the components of the assembly: ceil(L / step)
    cells per placed scaffold of size L > 0, in sequence order."""
    cell_first = np.full(len(sizes), -1, np.int64)
    seq_first = np.zeros(len(asm.components) + 1, np.int64)
    n = 0
    for q, comps in enumerate(asm.components):
        for s, _off, _orientation in comps:
            L = int(sizes[s])
            if L > 0:
                cell_first[s] = n
                n += -(-L // step)
        seq_first[q + 1] = n
    return cell_first, seq_first


def make_records(asm, sizes, step, cell_first, seq_first):
    """The records (lo, hi, q0, q1) of a report: per scaffold of two or more cells its interior boundaries, per pair of
    consecutive scaffolds of a sequence the slot of the junction.  Returns (int64[n, 4], {scaffold: row}, {(left, right): row})."""
    recs, of_scaffold, of_junction = [], {}, {}
    for q, comps in enumerate(asm.components):
        q0, q1 = int(seq_first[q]), int(seq_first[q + 1])
        filled = [s for s, _off, _o in comps if sizes[s] > 0]
        for k, s in enumerate(filled):
            first, n = int(cell_first[s]), -(-int(sizes[s]) // step)
            if n >= 2:
                of_scaffold[s] = len(recs)
                recs.append((first, first + n - 2, q0, q1))
            if k + 1 < len(filled):
                of_junction[(s, filled[k + 1])] = len(recs)
                recs.append((first + n - 1, first + n - 1, q0, q1))
    return np.asarray(recs, np.int64).reshape(-1, 4), of_scaffold, of_junction


def measure(ctx, pairFile, names, sizes, asm, step, maxSpan, flank, recs, threads, want_depth):
    """(stats4, cell_first, picks, counters, depth) through the array calls of a context the caller owns: the file is parsed on
    the host in chunks (hicmi_parse_valid_pairs) and marked chunk by chunk."""
    cell_first = ctx.span_begin(sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, step, maxSpan)
    stats = pairtool.parse_in_chunks(pairFile, names, sizes, threads, ctx.span_add_pairs)
    picks, counters, depth = ctx.span_finish(flank, recs, want_depth=want_depth)
    return stats, cell_first, picks, counters, depth


def pick_columns(pick, flank, minRatio, low, fine):
    """(depth, flank_depth, ratio, verdict) of a pick (slot, D, Lsum, Rsum) as text."""
    if pick is None or pick[0] < 0:
        return ["NA", "NA", "NA", "NA"]
    least = min(int(pick[2]), int(pick[3]))
    ratio = float(int(pick[1]) * flank) / float(least)
    return [str(int(pick[1])), repr(least / flank), repr(ratio), low if ratio < minRatio else fine]


def runPipeline(configFile, orderFile=None, scaffoldsOnly=False, gap=DEFAULT_GAP, step=DEFAULT_STEP, maxSpan=0, flank=DEFAULT_FLANK,
                minRatio=DEFAULT_MIN_RATIO, outFile=None, cutsFile=None, fullDir=None, threads=0, device=0, context=None):
    """``context``: a context of the caller's, driven through span_begin / span_add_pairs / span_finish; None: a context of
    its own on ``device`` and one pass of hicmi_span_file."""
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    if outFile is None:
        outFile = os.path.join(v["saveFilesDirectory"], "spanSupport.txt")
    with pairtool.refusing(OSError, ValueError):
        if step < 1:
            raise ValueError("the step %d is below 1" % step)
        if not 1 <= flank <= MAX_FLANK:
            raise ValueError("the flank %d is outside 1 .. %d" % (flank, MAX_FLANK))
        if maxSpan < 0:
            raise ValueError("maxSpan %d is negative" % maxSpan)
        if gap < 0:
            raise ValueError("the gap %d is negative" % gap)
        names, sizes = pairtool.read_scaffolds(v)
        if scaffoldsOnly:
            if orderFile is not None:
                raise ValueError("-scaffolds takes no order file")
            asm = identity_assembly(names, sizes)
        else:
            asm = pairtool.order_assembly(pairtool.resolve_order(v, orderFile), names, sizes, gap, chromosomes_only=False)
        n_cells = _lib.span_cell_count(sizes, asm.lift_seq, step)
        if n_cells > MAX_CELLS:
            raise ValueError("step %d cuts the assembly into %d cells, more than the %d a build can have" % (step, n_cells, MAX_CELLS))
        if n_cells < 1:
            raise ValueError("no scaffold of %s has a base" % v["hicProScaffSizeFile"])
    cell_first, seq_first = number_cells(asm, sizes, step)
    recs, of_scaffold, of_junction = make_records(asm, sizes, step, cell_first, seq_first)
    want_depth = fullDir is not None

    def count(ctx):
        if context is not None:
            return measure(ctx, v["validPairFile"], names, sizes, asm, step, maxSpan, flank, recs, threads, want_depth)
        return _lib.span_file(v["validPairFile"], names, sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, step, maxSpan, flank,
                              recs, ctx, threads=threads, want_depth=want_depth)

    stats, got_first, picks, counters, depth = pairtool.on_context(context, device, count)
    if not np.array_equal(got_first, cell_first):
        pairtool.refuse("the library numbers the cells differently from this report")
    stats = tuple(stats[:4])
    print(pairtool.lines_line("SPANS", stats) + ", " + pairtool.counted(COUNTER_COLUMNS, counters))

    def scaffold_line(s, orientation):
        L, cells = int(sizes[s]), (-(-int(sizes[s]) // step) if cell_first[s] >= 0 else 0)
        pick = picks[of_scaffold[s]] if s in of_scaffold else None
        cut = "NA"
        if pick is not None and pick[0] >= 0:
            inside = (int(pick[0]) - int(cell_first[s]) + 1) * step
            cut = str(L - inside if orientation == "-" else inside)
        cols = pick_columns(pick, flank, minRatio, "suspect", "spanned")
        return [names[s], orientation, str(L), str(cells), cut] + cols

    header = ["step=%d" % step, "maxSpan=%d" % maxSpan, "flank=%d" % flank, "minRatio=%r" % float(minRatio)]
    header += pairtool.fields(pairtool.STATS_COLUMNS, stats) + pairtool.fields(COUNTER_COLUMNS, counters.tolist())
    out = ["#" + "\t".join(header) + "\n", "#" + "\t".join(SCAFFOLD_COLUMNS) + "\n"]
    suspects, junctions = [], []
    n_listed = len(asm.components) if scaffoldsOnly else asm.n_chromosomes
    for q, comps in enumerate(asm.components):
        if scaffoldsOnly:
            if q == 0:
                out.append("### Scaffolds ###\n")
        elif q < n_listed:
            out.append("### Chromosome grouping %d ###\n" % (q + 1))
        elif q == n_listed:
            break
        for s, _off, orientation in comps:
            cols = scaffold_line(s, orientation)
            out.append("\t".join(cols) + "\n")
            if cols[-1] == "suspect":
                suspects.append((cols[0], cols[4], cols[7]))
        filled = [s for s, _off, _o in comps if sizes[s] > 0]
        for left, right in zip(filled, filled[1:]):
            cols = pick_columns(picks[of_junction[(left, right)]], flank, minRatio, "weak", "held")
            junctions.append("\t".join([str(q + 1), names[left], names[right]] + cols) + "\n")
    if not scaffoldsOnly:
        out += ["### Junctions ###\n", "#" + "\t".join(JUNCTION_COLUMNS) + "\n"] + junctions + ["### Unplaced ###\n"]
        for comps in asm.components[n_listed:]:
            for s, _off, orientation in comps:
                cols = scaffold_line(s, orientation)
                out.append("\t".join(cols) + "\n")
                if cols[-1] == "suspect":
                    suspects.append((cols[0], cols[4], cols[7]))
    pairtool.write_text(outFile, "".join(out), mkdir=True)
    if cutsFile is not None:
        pairtool.write_text(cutsFile, "".join("%s\t%s\t%s\n" % row for row in suspects))
    if fullDir is not None:
        os.makedirs(fullDir, exist_ok=True)
        with open(os.path.join(fullDir, "spans.depth.tsv"), "w") as fh:
            fh.write("#sequence\tfirst_base\tlast_base\tdepth\n")
            for name, comps in zip(asm.seq_names, asm.components):
                for s, off, _orientation in comps:
                    L = int(sizes[s])
                    for j in range(-(-L // step) if cell_first[s] >= 0 else 0):
                        fh.write("%s\t%d\t%d\t%d\n" % (name, off + j * step + 1, off + min((j + 1) * step, L), int(depth[cell_first[s] + j])))
    print("SPANS: %d scaffold(s) suspect, %d of %d junction(s) weak" % (len(suspects), sum(j.endswith("\tweak\n") for j in junctions),
                                                                        len(junctions)))
    return stats, picks, counters, suspects


def main(argv=None, context=None):
    parser = argparse.ArgumentParser(description="Counts, on the GPU, the read pairs of validPairFile that span every cut of every "
                                                 "scaffold and every junction of an ordering, and reports where the depth dips.")
    with pairtool.common_arguments(parser):
        parser.add_argument("-scaffolds", help="Every scaffold on its own: no order file, only cuts are reported", action="store_true")
        parser.add_argument("-gap", help="Bases between neighbouring scaffolds (default %d, as Part 4 writes)" % DEFAULT_GAP, type=int,
                            default=DEFAULT_GAP)
        parser.add_argument("-step", help="Cell size in bp (default %d)" % DEFAULT_STEP, type=int, default=DEFAULT_STEP)
        parser.add_argument("-maxSpan", help="Longest distance of a pair that counts, in bp (default 0: no limit)", type=int, default=0)
        parser.add_argument("-flank", help="Cells of each flank (default %d)" % DEFAULT_FLANK, type=int, default=DEFAULT_FLANK)
        parser.add_argument("-minRatio", help="Ratio below which a cut is suspect and a junction weak (default %r)" % DEFAULT_MIN_RATIO,
                            type=float, default=DEFAULT_MIN_RATIO)
        parser.add_argument("-out", help="Report (default: saveFilesDirectory/spanSupport.txt)", type=str, default=None)
        parser.add_argument("-cuts", help="Write scaffold, cut_after and ratio of every suspect scaffold to this file", type=str, default=None)
        parser.add_argument("-full", help="Write spans.depth.tsv, the depth of every cell, into this directory", type=str, default=None)
    args = parser.parse_args(argv)
    return runPipeline(args.config, args.order, args.scaffolds, args.gap, args.step, args.maxSpan, args.flank, args.minRatio, args.out,
                       args.cuts, args.full, threads=args.threads, device=args.device, context=context)


if __name__ == "__main__":
    main()
