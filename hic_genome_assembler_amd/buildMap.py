"""Raw contact maps at any resolution from HiC-Pro's valid pairs, on the device.

The bin grid of every other stage comes from a HiC-Pro ``build_matrix`` run made hours earlier; rebinMap reaches only the
integer multiples of that run's bin size.  ``validPairFile`` - the allValidPairs file Part 3 reads - holds everything
needed to count the raw map at any bin size: HiC-Pro cuts every scaffold of ``hicProScaffSizeFile`` into bins from its own
start (hostio.bins_from_sizes), a read pair adds 1 to the cell of the two bins its ends fall in, and one pass over the
file counts the maps of all resolutions asked for (``hicmi_build_maps``: the file is parsed once in chunks by the
library's multi-threaded parser, every chunk is uploaded once and counted into every map).  Each map is then balanced
(``-part0``'s ICE, iceNormalize.balanceResident) and written as the file set rebinMap writes, ready for
``run_hicAssembler.py -part1 -part2``:

    python -m hic_genome_assembler_amd.buildMap -config my_config.txt -resolution 100000,150000,250000 \\
           [-out DIR] [-noBalance] [-threads 0] [-device 0]

Per resolution r, in ``DIR/res<r>/`` (DIR: ``saveFilesDirectory/build``): ``build_<r>_abs.bed``, the raw
``build_<r>.matrix``, unless ``-noBalance`` ``build_<r>_iced.matrix`` and its ``.biases``, and ``config.txt`` - the input
config with the resolution, the four HiC-Pro files that depend on it and the two output directories replaced, every other
line verbatim; the config's own ``resolution`` need not be one of those asked for.  ``DIR/build_summary.tsv`` has one
line per resolution after a comment line with the file's statistics: lines, pairs used, lines naming a scaffold that is
not in the size file, lines with a position outside its scaffold (both kinds are skipped).
"""
from __future__ import annotations

import argparse
import os
import sys

from . import _lib
from .hostio import bins_from_sizes, count_bins, paused_gc, read_scaffold_sizes
from .rebinMap import output_paths, scaffold_counts, write_resolution

MAX_BINS = 65536                                # the context's limit (hicmi_set_contacts_*)
SUMMARY_COLUMNS = ("resolution", "bins", "scaffolds", "one_bin_scaffolds", "masked_scaffold_size", "masked_no_counts",
                   "masked_low_counts", "iterations", "final_delta", "read_pairs")
STATS_COLUMNS = ("lines", "used", "unknown_scaffold", "out_of_range")


def parse_resolutions(text):
    """``-resolution``'s value, "100000,150000": the resolutions in the order given.  ValueError for anything but distinct
    integers from 1 on."""
    out = []
    for part in str(text).split(","):
        try:
            r = int(part.strip())
        except ValueError:
            raise ValueError("-resolution must be a comma-separated list of integers, got %r" % part.strip())
        if r < 1:
            raise ValueError("resolution %d is below 1" % r)
        if r in out:
            raise ValueError("resolution %d is given twice" % r)
        out.append(r)
    return out


def check_valid_pair_file(path):
    """ValueError unless ``path`` is a file to read pairs from (the synthetic configs set ``/dev/null``)."""
    if not path or not os.path.exists(path):
        raise ValueError("validPairFile %r does not exist" % path)
    if os.path.samefile(path, os.devnull) or not os.path.isfile(path):
        raise ValueError("validPairFile %s is not a file of read pairs" % path)


def runPipeline(configFile, resolutions, outDir=None, balance=True, threads=0, device=0):
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    ice = driver.iceSettings(v)
    if outDir is None:
        outDir = os.path.join(v["saveFilesDirectory"], "build")
    try:
        check_valid_pair_file(v["validPairFile"])
        names, sizes = read_scaffold_sizes(v["hicProScaffSizeFile"])
        if not names:
            raise ValueError("hicProScaffSizeFile %s lists no scaffold" % v["hicProScaffSizeFile"])
        for r in resolutions:
            m = count_bins(sizes, r)
            if m > MAX_BINS:
                raise ValueError("resolution %d needs %d bins, more than the %d a map can have" % (r, m, MAX_BINS))
    except (OSError, ValueError) as exc:
        sys.exit("ERROR... %s. Exiting..." % exc)
    rows = []
    with paused_gc():
        ctxs = [_lib.Context(device) for _r in resolutions]
        try:
            try:
                stats = _lib.build_maps(v["validPairFile"], names, sizes, resolutions, ctxs, threads=threads)
            except _lib.HicmiError as exc:
                sys.exit("ERROR... %s. Exiting..." % exc)
            print("BUILD: lines %d, pairs used %d, unknown scaffold %d, out of range %d, chunks %d" % stats)
            if stats[3]:
                print("WARNING... %d line(s) of %s have a position below 1 or beyond the size of their scaffold in %s and were "
                      "skipped: do the two files belong to one assembly?" % (stats[3], v["validPairFile"], v["hicProScaffSizeFile"]))
            for r, ctx in zip(resolutions, ctxs):
                binList = bins_from_sizes((names, sizes), r)
                paths = output_paths(outDir, r, prefix="build")
                n_scaf, n_one = scaffold_counts(binList)
                line = "BUILD: resolution %d, bins %d (scaffolds %d, of one bin %d)" % (r, len(binList), n_scaf, n_one)
                ice_cols, pairs = write_resolution(ctx, binList, paths, configFile, v, ice, balance, line)
                rows.append([str(r), str(len(binList)), str(n_scaf), str(n_one)] + ice_cols + [repr(pairs)])
                ctx.close()                                             # its map is written: the memory goes back now
        finally:
            for ctx in ctxs:
                ctx.close()
    with open(os.path.join(os.path.abspath(outDir), "build_summary.tsv"), "w") as fh:
        fh.write("#" + "\t".join("%s=%d" % kv for kv in zip(STATS_COLUMNS, stats)) + "\n")
        fh.write("#" + "\t".join(SUMMARY_COLUMNS) + "\n")
        fh.write("".join("\t".join(r) + "\n" for r in rows))
    return rows, stats


def main(argv=None):
    parser = argparse.ArgumentParser(description="Counts the raw contact map at every resolution asked for from HiC-Pro's valid "
                                                 "pairs (validPairFile) on the GPU and balances each, ready for -part1 -part2.")
    parser.add_argument("-config", help="Full file path to the config file", required=True, type=str)
    parser.add_argument("-resolution", help="Comma-separated bin sizes in bp: one output per resolution", required=True, type=str)
    parser.add_argument("-out", help="Output directory (default: saveFilesDirectory/build)", type=str, default=None)
    parser.add_argument("-noBalance", help="Write the bed file and the raw map only, no ICE", action="store_true")
    parser.add_argument("-threads", help="Host threads of the parser (default 0: all)", type=int, default=0)
    parser.add_argument("-device", help="GPU index (default 0)", type=int, default=0)
    args = parser.parse_args(argv)
    try:
        resolutions = parse_resolutions(args.resolution)
    except ValueError as exc:
        sys.exit("ERROR... %s. Exiting..." % exc)
    runPipeline(args.config, resolutions, args.out, balance=not args.noBalance, threads=args.threads, device=args.device)


if __name__ == "__main__":
    main()
