"""Refinement of an existing Part 2 ordering: the best relocation or segment inversion applied, round by round.

    python -m hic_genome_assembler_amd.refinePart2 -config cfg.txt [-chromosomeOrderFile FILE] [-out DIR]
           [-moves relocate,invert] [-maxSpan 0] [-minGain 0] [-maxRounds 100] [-device 0]

Reads the config's chromosomeGroupFile and a chromosomeOrderFile (the config's by default), loads the map once and climbs
(orderGenome.refineOrdering): every round builds, for all chromosomes that have not converged, the
placement table of supportPart2 and the inversion table of supportInversions, takes each scaffold's decided best
relocation and each left end's decided best inversion with their literal score deltas, and applies the first strict
maximum of them (relocations before inversions) if it is > 0 and > minGain * |score0|; a chromosome without such a move
has converged.  One move per chromosome per round.  ``-moves`` selects the families, ``-maxSpan N`` bounds the inverted
segments to N scaffolds, ``-maxRounds`` caps the loop (a chromosome stopped by the cap is reported as not converged).

Written to ``-out DIR`` (default saveFilesDirectory/refined): the refined chromosomeOrderFile and plotOrderFile under
their config names, ``refine.log`` (one line per applied move: round, chromosome, kind, scaffold(s), from -> to, score
before, score after) and ``refine_summary.tsv`` (per chromosome: score before and after, moves, rounds, converged).  The
input order file is never changed.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

from . import orderGenome as p2
from .run_hicAssembler import ensureAllVariablesAreSet, readConfigFileToVariables
from .supportPart2 import reportOnOrderFile


def parse_moves(text):
    """``relocate,invert`` as a tuple of families, in REFINE_MOVES' order; ValueError for anything else."""
    names = [t.strip() for t in text.split(",") if t.strip()]
    if not names or any(t not in p2.REFINE_MOVES for t in names):
        raise ValueError("-moves takes a comma-separated list of " + ", ".join(p2.REFINE_MOVES))
    return tuple(m for m in p2.REFINE_MOVES if m in names)


def runRefine(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile,
              outDir, moves=p2.REFINE_MOVES, maxSpan=0, minGain=0.0, maxRounds=100, device=0):
    """The refinement of ``chromosomeOrderFile`` written to ``outDir``; returns (refined ordering, log, summary)."""
    t0 = time.time()
    target = os.path.join(outDir, os.path.basename(chromosomeOrderFile))
    if os.path.abspath(target) == os.path.abspath(chromosomeOrderFile):
        raise ValueError("the refined order file must not be the input order file itself")

    def report(matrix, ordered, binList, chromList):
        out = p2.refineOrdering(matrix, ordered, binList, chromList, moves=moves, maxSpan=maxSpan, minGain=minGain,
                                maxRounds=maxRounds)
        p2.writeRefinement(*out, outDir, chromosomeOrderFile, plotOrderFile)
        return out
    out = reportOnOrderFile(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, device,
                            report)
    print("Total run-time of the refinement = " + str(time.time() - t0))
    return out


def _parse_args(argv):
    p = argparse.ArgumentParser(description="Hill-climbing refinement of a finished Part 2 ordering: the best relocation "
                                            "or segment inversion of every chromosome applied round by round, on one GPU.")
    p.add_argument("-config", required=True, type=str, help="run_hicAssembler.py config file")
    p.add_argument("-chromosomeOrderFile", type=str, default=None, help="order file to refine (default: the config's)")
    p.add_argument("-out", type=str, default=None, help="output directory (default: saveFilesDirectory/refined)")
    p.add_argument("-moves", type=str, default=",".join(p2.REFINE_MOVES), help="move families (default relocate,invert)")
    p.add_argument("-maxSpan", type=int, default=0, help="most scaffolds in an inverted segment (default 0: no limit)")
    p.add_argument("-minGain", type=float, default=0.0, help="least gain of a move, relative to |score0| (default 0)")
    p.add_argument("-maxRounds", type=int, default=100, help="most rounds (default 100)")
    p.add_argument("-device", type=int, default=0, help="GPU index (default 0)")
    return p.parse_args(argv)


def resolve(args, v):
    """(order file, output directory, move families) of a command line and its config."""
    order = args.chromosomeOrderFile or v["chromosomeOrderFile"]
    out = args.out or os.path.join(v["saveFilesDirectory"], "refined")
    return order, out, parse_moves(args.moves)


def main(argv=None):
    args = _parse_args(argv)
    if args.maxSpan < 0 or args.maxRounds < 1 or args.minGain < 0:
        sys.exit("-maxSpan and -minGain must not be negative and -maxRounds must be at least 1")
    v = readConfigFileToVariables(args.config)
    if ensureAllVariablesAreSet(v):
        sys.exit(2)
    try:
        order, out, moves = resolve(args, v)
    except ValueError as e:
        sys.exit(str(e))
    runRefine(v["hicProBedFile"], v["hicProBiasFile"], v["hicProMatrixFile"], v["chromosomeGroupFile"], order,
              v["plotOrderFile"], out, moves=moves, maxSpan=args.maxSpan, minGain=args.minGain, maxRounds=args.maxRounds,
              device=args.device)


if __name__ == "__main__":
    main()
