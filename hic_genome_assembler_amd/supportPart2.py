"""Placement support of an existing Part 2 ordering: which scaffolds the map holds firmly in place.

    python -m hic_genome_assembler_amd.supportPart2 -config cfg.txt [-chromosomeOrderFile FILE] [-out FILE] [-full DIR]
           [-device 0]

Reads the config's chromosomeGroupFile and a chromosomeOrderFile (the config's by default; one written by ``-part2``, by
``sweepPart2`` or by the reference), loads the map once (the grouped bins only, as ``-part2`` reads it) and takes every
scaffold out of its chromosome's arrangement and puts it back at every gap in both orientations
(orderGenome.placementSupport).  The report - ``### Chromosome grouping i ### score0`` and one line per
scaffold: scaffold, orientation, bins, flip_delta, best_gap, best_orientation, best_delta, verdict - goes to ``-out``
(default: the config's placementSupportFile, else saveFilesDirectory/placementSupport.txt).  ``-full DIR`` also writes each
chromosome's S x 2S score table as ``DIR/Chr_i.support.tsv``.

Verdicts: ``improvable`` - some other placement scores higher (the search is a heuristic: a finding, not an error);
``orientation_open`` - flipping the scaffold in place changes nothing (one-bin scaffolds: Part 3's candidates);
``supported`` otherwise.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

from . import orderGenome as p2
from .hostio import initiateLoci, paused_gc
from .run_hicAssembler import ensureAllVariablesAreSet, readConfigFileToVariables


def reportOnOrderFile(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, device,
                      report):
    """What runSupport and supportBreaks.runBreaks share: the map of the grouped bins loaded once, the group file and the
    order file read, and ``report(matrix, ordered chromosomes, binList, chromList)`` returned."""
    binDict = p2.readGroupingsToValidBins(chromosomeGroupFile)
    binList = initiateLoci(hicProBedFile, hicProBiasFile, binID_dict=binDict)
    matrix = p2.buildAdjacencyMatrix(hicProMatrixFile, binList, device=device)
    try:
        with paused_gc():
            chromList = p2.readChromsFromFile(chromosomeGroupFile)
            ordered = p2.scaffoldsFromOrderFile(chromList, chromosomeOrderFile)
            return report(matrix, ordered, binList, chromList)
    finally:
        matrix.ctx.close()


def runSupport(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, outFile,
               fullDir=None, device=0):
    """The report for ``chromosomeOrderFile`` written to ``outFile``; returns placementSupport's results."""
    t0 = time.time()

    def report(matrix, ordered, binList, chromList):
        results = p2.placementSupport(matrix, ordered, binList, chromList)
        p2.writePlacementSupportToFile(results, outFile, fullDir)
        return results
    results = reportOnOrderFile(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile,
                                device, report)
    print("Total run-time of the placement support = " + str(time.time() - t0))
    return results


def _parse_args(argv):
    p = argparse.ArgumentParser(description="Placement support of a finished Part 2 ordering: every scaffold re-placed "
                                            "at every gap in both orientations, on one GPU.")
    p.add_argument("-config", required=True, type=str, help="run_hicAssembler.py config file")
    p.add_argument("-chromosomeOrderFile", type=str, default=None,
                   help="order file to assess (default: the config's), e.g. a sweep's best/ or the reference's")
    p.add_argument("-out", type=str, default=None,
                   help="report file (default: the config's placementSupportFile, else saveFilesDirectory/placementSupport.txt)")
    p.add_argument("-full", type=str, default=None, help="directory for each chromosome's S x 2S score table (TSV)")
    p.add_argument("-device", type=int, default=0, help="GPU index (default 0)")
    return p.parse_args(argv)


def resolve(args, v):
    """(order file, report file) of a command line and its config."""
    order = args.chromosomeOrderFile or v["chromosomeOrderFile"]
    out = args.out or v.get("placementSupportFile") or os.path.join(v["saveFilesDirectory"], "placementSupport.txt")
    return order, out


def main(argv=None):
    args = _parse_args(argv)
    v = readConfigFileToVariables(args.config)
    if ensureAllVariablesAreSet(v):
        sys.exit(2)
    order, out = resolve(args, v)
    runSupport(v["hicProBedFile"], v["hicProBiasFile"], v["hicProMatrixFile"], v["chromosomeGroupFile"], order, out,
               fullDir=args.full, device=args.device)


if __name__ == "__main__":
    main()
