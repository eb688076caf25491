"""Break support of an existing Part 2 ordering: where the map would rather have a scaffold cut.

    python -m hic_genome_assembler_amd.supportBreaks -config cfg.txt [-chromosomeOrderFile FILE] [-out FILE]
           [-broken FILE] [-minPiece 1] [-full DIR] [-device 0]

Reads the config's chromosomeGroupFile and a chromosomeOrderFile (the config's by default; one written by ``-part2``, by
``sweepPart2`` or by the reference), loads the map once (the grouped bins only, as ``-part2`` reads it) and cuts every
scaffold between every two of its bins: the two pieces are swapped and / or reversed in place, 8 candidates per cut
(orderGenome.breakSupport).  The report - ``### Chromosome grouping i ### score0`` and one line per
scaffold: scaffold, orientation, bins, best_cut, cut_after_bin, best_move, best_delta, gain, verdict - goes to ``-out``
(default: the config's breakSupportFile, else saveFilesDirectory/breakSupport.txt).  ``-broken FILE`` (default: the
config's brokenChromosomeGroupFile, else none) writes the group file with every ``breakable`` scaffold split into
``NAME.brk1`` and ``NAME.brk2`` at its best cut; ``-part2`` on that file orders the pieces independently.  ``-minPiece N``:
only cuts that leave both pieces at least N bins compete.  ``-full DIR`` also writes each chromosome's table of scores as
``DIR/Chr_i.breaks.tsv``, one line per (scaffold, cut).

Verdicts: ``breakable`` - some rearrangement of the two pieces scores higher than the scaffold as it lies (a finding
about the primary assembly, for a person to look at); ``intact`` - none does; ``NA`` - no candidate (one or two bins, or
no cut leaves two pieces of minPiece bins).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

from . import orderGenome as p2
from .run_hicAssembler import ensureAllVariablesAreSet, readConfigFileToVariables
from .supportPart2 import reportOnOrderFile


def runBreaks(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, outFile,
              brokenFile=None, minPiece=1, fullDir=None, device=0):
    """The report for ``chromosomeOrderFile`` written to ``outFile`` (and the broken group file to ``brokenFile``);
    returns breakSupport's results."""
    t0 = time.time()
    results = reportOnOrderFile(
        hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, device,
        lambda matrix, ordered, binList, chromList: p2.breakSupportToFiles(
            matrix, ordered, binList, chromosomeGroupFile, outFile, brokenFile, fullDir=fullDir, minPiece=minPiece,
            chromList=chromList))
    print("Total run-time of the break support = " + str(time.time() - t0))
    return results


def _parse_args(argv):
    p = argparse.ArgumentParser(description="Break support of a finished Part 2 ordering: every scaffold cut at every "
                                            "bin boundary, the pieces swapped and reversed in place, on one GPU.")
    p.add_argument("-config", required=True, type=str, help="run_hicAssembler.py config file")
    p.add_argument("-chromosomeOrderFile", type=str, default=None,
                   help="order file to assess (default: the config's), e.g. a sweep's best/ or the reference's")
    p.add_argument("-out", type=str, default=None,
                   help="report file (default: the config's breakSupportFile, else saveFilesDirectory/breakSupport.txt)")
    p.add_argument("-broken", type=str, default=None,
                   help="group file with the breakable scaffolds split (default: the config's brokenChromosomeGroupFile, "
                        "else not written)")
    p.add_argument("-minPiece", type=int, default=1, help="fewest bins of a piece for a cut to compete (default 1)")
    p.add_argument("-full", type=str, default=None, help="directory for each chromosome's table of scores (TSV)")
    p.add_argument("-device", type=int, default=0, help="GPU index (default 0)")
    return p.parse_args(argv)


def resolve(args, v):
    """(order file, report file, broken group file or None) of a command line and its config."""
    order = args.chromosomeOrderFile or v["chromosomeOrderFile"]
    out = args.out or v.get("breakSupportFile") or os.path.join(v["saveFilesDirectory"], "breakSupport.txt")
    broken = args.broken or v.get("brokenChromosomeGroupFile") or None
    return order, out, broken


def main(argv=None):
    args = _parse_args(argv)
    v = readConfigFileToVariables(args.config)
    if ensureAllVariablesAreSet(v):
        sys.exit(2)
    order, out, broken = resolve(args, v)
    runBreaks(v["hicProBedFile"], v["hicProBiasFile"], v["hicProMatrixFile"], v["chromosomeGroupFile"], order, out,
              brokenFile=broken, minPiece=args.minPiece, fullDir=args.full, device=args.device)


if __name__ == "__main__":
    main()
