"""Inversion support of an existing Part 2 ordering: which runs of scaffolds the map would rather read backwards.

    python -m hic_genome_assembler_amd.supportInversions -config cfg.txt [-chromosomeOrderFile FILE] [-out FILE]
           [-maxSpan 0] [-full DIR] [-device 0]

Reads the config's chromosomeGroupFile and a chromosomeOrderFile (the config's by default; one written by ``-part2``, by
``sweepPart2`` or by the reference), loads the map once (the grouped bins only, as ``-part2`` reads it) and reverses every
run of consecutive scaffolds i ... j of every chromosome: reverse order, every orientation flipped
(orderGenome.inversionSupport).  Part 2's windows see at most 8 scaffolds, so a longer block lying the
wrong way round is invisible to them.  The report - ``### Chromosome grouping i ### score0`` and one line per scaffold,
as the left end of a segment: scaffold, orientation, bins, best_end, span, span_bins, best_delta, gain, verdict - goes to
``-out`` (default: the config's inversionSupportFile, else saveFilesDirectory/inversionSupport.txt).  ``-maxSpan N``: only
segments of at most N scaffolds are computed and compete (0: all).  ``-full DIR`` also writes each chromosome's S x S
table of scores as ``DIR/Chr_i.inversions.tsv`` (row = first scaffold, column = last).

Verdicts: ``invertible`` - the best segment that starts here scores higher reversed (refinePart2 applies such moves);
``supported`` - none does; ``NA`` - nothing competes (the last scaffold, a chromosome of one or two scaffolds).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

from . import orderGenome as p2
from .run_hicAssembler import ensureAllVariablesAreSet, readConfigFileToVariables
from .supportPart2 import reportOnOrderFile


def runInversions(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, outFile,
                  maxSpan=0, fullDir=None, device=0):
    """The report for ``chromosomeOrderFile`` written to ``outFile``; returns inversionSupport's results."""
    t0 = time.time()

    def report(matrix, ordered, binList, chromList):
        results = p2.inversionSupport(matrix, ordered, binList, chromList, maxSpan=maxSpan)
        p2.writeInversionSupportToFile(results, outFile, fullDir)
        return results
    results = reportOnOrderFile(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile,
                                device, report)
    print("Total run-time of the inversion support = " + str(time.time() - t0))
    return results


def _parse_args(argv):
    p = argparse.ArgumentParser(description="Inversion support of a finished Part 2 ordering: every run of consecutive "
                                            "scaffolds reversed and flipped, on one GPU.")
    p.add_argument("-config", required=True, type=str, help="run_hicAssembler.py config file")
    p.add_argument("-chromosomeOrderFile", type=str, default=None,
                   help="order file to assess (default: the config's), e.g. a sweep's best/ or the reference's")
    p.add_argument("-out", type=str, default=None,
                   help="report file (default: the config's inversionSupportFile, else saveFilesDirectory/inversionSupport.txt)")
    p.add_argument("-maxSpan", type=int, default=0, help="most scaffolds in a segment (default 0: no limit)")
    p.add_argument("-full", type=str, default=None, help="directory for each chromosome's S x S table of scores (TSV)")
    p.add_argument("-device", type=int, default=0, help="GPU index (default 0)")
    return p.parse_args(argv)


def resolve(args, v):
    """(order file, report file) of a command line and its config."""
    order = args.chromosomeOrderFile or v["chromosomeOrderFile"]
    out = args.out or v.get("inversionSupportFile") or os.path.join(v["saveFilesDirectory"], "inversionSupport.txt")
    return order, out


def main(argv=None):
    args = _parse_args(argv)
    if args.maxSpan < 0:
        sys.exit("-maxSpan must be 0 (no limit) or a positive number of scaffolds")
    v = readConfigFileToVariables(args.config)
    if ensureAllVariablesAreSet(v):
        sys.exit(2)
    order, out = resolve(args, v)
    runInversions(v["hicProBedFile"], v["hicProBiasFile"], v["hicProMatrixFile"], v["chromosomeGroupFile"], order, out,
                  maxSpan=args.maxSpan, fullDir=args.full, device=args.device)


if __name__ == "__main__":
    main()
