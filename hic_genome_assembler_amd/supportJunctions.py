"""Junction support of an existing Part 2 ordering: which chromosome ends belong together, which junctions do not hold.

    python -m hic_genome_assembler_amd.supportJunctions -config cfg.txt [-chromosomeOrderFile FILE] [-out FILE]
           [-window 16] [-minRel 0.25] [-joined DIR] [-cut DIR] [-full DIR] [-device 0]

Reads the config's chromosomeGroupFile and a chromosomeOrderFile (the config's by default; one written by ``-part2``, by
``sweepPart2`` or by the reference), loads the map once (the grouped bins only, as ``-part2`` reads it) and measures the
mean contact, weighted 1 / distance, across every scaffold boundary of every chromosome and between every two ends of
different chromosomes (orderGenome.junctionSupport).  Part 1 cuts a chromosome into several groups far
more often than it merges two; Part 2 then orders each piece as a chromosome of its own.  The report -
``### reference ref window W minRel r``, per chromosome one line per internal junction (left scaffold, right scaffold,
bins_left, bins_right, J, rel, verdict), then ``### Chromosome ends ###`` and one line per end (chromosome, head/tail,
terminal scaffold, bins, best_chromosome, best_end, J, rel, mutual, second_chromosome, second_J, verdict) - goes to
``-out`` (default: the config's junctionSupportFile, else saveFilesDirectory/junctionSupport.txt).  ``-window N``: a
side is its first N bins (0: the whole block).  ``-full DIR`` also writes the table of J between all ends as
``DIR/junctions.ends.tsv``.

Verdicts: an end is ``joinable`` when it and its best partner choose each other and their J is at least ``-minRel`` times
the median internal junction, else ``free``; an internal junction is ``held`` at or above that bound, else ``weak``.
``-joined DIR`` writes the group, order and plot-order files with every joinable pair joined (and ``joins.log``),
``-cut DIR`` the same files with every chromosome split at its weak junctions (and ``cuts.log``), under the names the
config gives those files: a valid input to supportPart2, supportInversions, refinePart2, ``-part2`` and Part 4.  The
input files are never changed.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

from . import orderGenome as p2
from .run_hicAssembler import ensureAllVariablesAreSet, readConfigFileToVariables
from .supportPart2 import reportOnOrderFile


def runJunctions(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, outFile,
                 plotOrderFile=None, window=p2.JUNCTION_WINDOW, minRel=p2.JUNCTION_MIN_REL, joinedDir=None, cutDir=None,
                 fullDir=None, device=0):
    """The report for ``chromosomeOrderFile`` written to ``outFile``; returns junctionSupport's results.
    ``plotOrderFile`` names the plot-order file of ``joinedDir`` / ``cutDir`` (default: plotOrder.txt)."""
    t0 = time.time()
    plotOrderFile = plotOrderFile or os.path.join(os.path.dirname(chromosomeOrderFile), "plotOrder.txt")

    def report(matrix, ordered, binList, chromList):
        return p2.junctionSupportToFiles(matrix, ordered, binList, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile,
                                         outFile, joinedDir, cutDir, fullDir, window=window, minRel=minRel)
    results = reportOnOrderFile(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile,
                                device, report)
    print("Total run-time of the junction support = " + str(time.time() - t0))
    return results


def _parse_args(argv):
    p = argparse.ArgumentParser(description="Junction support of a finished Part 2 ordering: the contact across every "
                                            "scaffold boundary and between every two chromosome ends, on one GPU.")
    p.add_argument("-config", required=True, type=str, help="run_hicAssembler.py config file")
    p.add_argument("-chromosomeOrderFile", type=str, default=None,
                   help="order file to assess (default: the config's), e.g. a sweep's best/ or the reference's")
    p.add_argument("-out", type=str, default=None,
                   help="report file (default: the config's junctionSupportFile, else saveFilesDirectory/junctionSupport.txt)")
    p.add_argument("-window", type=int, default=p2.JUNCTION_WINDOW, help="bins of a side (default 16; 0: the whole block)")
    p.add_argument("-minRel", type=float, default=p2.JUNCTION_MIN_REL,
                   help="J / median internal J at or above which a junction holds (default 0.25)")
    p.add_argument("-joined", type=str, default=None, help="directory for the files with the joinable ends joined")
    p.add_argument("-cut", type=str, default=None, help="directory for the files with the weak junctions cut")
    p.add_argument("-full", type=str, default=None, help="directory for the table of J between all chromosome ends (TSV)")
    p.add_argument("-device", type=int, default=0, help="GPU index (default 0)")
    return p.parse_args(argv)


def resolve(args, v):
    """(order file, report file) of a command line and its config."""
    order = args.chromosomeOrderFile or v["chromosomeOrderFile"]
    out = args.out or v.get("junctionSupportFile") or os.path.join(v["saveFilesDirectory"], "junctionSupport.txt")
    return order, out


def main(argv=None):
    args = _parse_args(argv)
    if args.window < 0:
        sys.exit("-window must be 0 (the whole block) or a positive number of bins")
    if not args.minRel > 0:
        sys.exit("-minRel must be above 0")
    if args.joined and args.cut and os.path.abspath(args.joined) == os.path.abspath(args.cut):
        sys.exit("-joined and -cut need directories of their own: joins and cuts are never applied in one file")
    v = readConfigFileToVariables(args.config)
    if ensureAllVariablesAreSet(v):
        sys.exit(2)
    order, out = resolve(args, v)
    runJunctions(v["hicProBedFile"], v["hicProBiasFile"], v["hicProMatrixFile"], v["chromosomeGroupFile"], order, out,
                 plotOrderFile=v["plotOrderFile"], window=args.window, minRel=args.minRel, joinedDir=args.joined,
                 cutDir=args.cut, fullDir=args.full, device=args.device)


if __name__ == "__main__":
    main()
