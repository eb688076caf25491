"""Coarser resolutions from one raw HiC-Pro map, on the device.

The reference's README calls the resolution the setting that matters most ("a resolution size of 100-500Kb"), and it is
the one setting fixed hours earlier, by the HiC-Pro run that cut the reads into bins.  HiC-Pro bins every scaffold from
its own start, so the bins of a map at k times the bin size are the runs of k consecutive bins of one scaffold, and its
raw counts are sums of blocks of the fine raw map (``hicmi_rebin``) - with the one exception of the diagonal, where the
pairs between two fine bins that fall into one coarse bin become pairs inside a bin and are counted once.  So one fine
raw map gives every coarser one, each balanced (``-part0``'s ICE, iceNormalize.balanceResident) and ready for
``run_hicAssembler.py -part1 -part2``:

    python -m hic_genome_assembler_amd.rebinMap -config my_config.txt -factor 2,3,5 [-out DIR] [-noBalance] [-device 0]

The bed file and ``hicProRawMatrixFile`` are read once and the fine map is uploaded once; per factor a second context
adopts it, rebins and balances.  Per factor, in ``DIR/res<k * resolution>/`` (DIR: ``saveFilesDirectory/rebin``): the bed
file, the raw ``.matrix``, unless ``-noBalance`` the ``_iced.matrix`` and its ``.biases`` (one line per bed line, ``nan``
for the bins ICE masked), and ``config.txt`` - the input config with the resolution, the four HiC-Pro files that depend
on it and the two output directories replaced, every other line verbatim.  ``DIR/rebin_summary.tsv`` has one line per
factor; the one-bin scaffolds it counts are those Part 2 cannot orient - the price of coarsening.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from . import _lib
from .hostio import paused_gc, read_bed_bins, read_contact_matrix, rebin_bins, write_bed, write_biases, write_iced_matrix

MAX_FACTOR = 64                                 # hicmi_rebin: fine bins per coarse bin
REWRITTEN_KEYS = ("resolution", "hicProBedFile", "hicProMatrixFile", "hicProBiasFile", "hicProRawMatrixFile",
                  "saveFilesDirectory", "savePlotsDirectory")
SUMMARY_COLUMNS = ("factor", "resolution", "bins", "scaffolds", "one_bin_scaffolds", "masked_scaffold_size",
                   "masked_no_counts", "masked_low_counts", "iterations", "final_delta", "read_pairs")


def parse_factors(text):
    """``-factor``'s value, "2,3,5": the factors in the order given.  ValueError for anything but distinct integers in
    2 .. 64."""
    factors = []
    for part in str(text).split(","):
        try:
            k = int(part.strip())
        except ValueError:
            raise ValueError("-factor must be a comma-separated list of integers, got %r" % part.strip())
        if k < 2 or k > MAX_FACTOR:
            raise ValueError("factor %d is outside 2 .. %d" % (k, MAX_FACTOR))
        if k in factors:
            raise ValueError("factor %d is given twice" % k)
        factors.append(k)
    return factors


def output_paths(outDir, resolution, prefix="rebin"):
    """The files of one resolution, keyed by the config keys they are written under (plus the directory)."""
    d = os.path.join(os.path.abspath(outDir), "res%d" % resolution)
    stem = os.path.join(d, "%s_%d" % (prefix, resolution))
    return {"dir": d, "resolution": str(resolution), "hicProBedFile": stem + "_abs.bed", "hicProRawMatrixFile": stem + ".matrix",
            "hicProMatrixFile": stem + "_iced.matrix", "hicProBiasFile": stem + "_iced.matrix.biases",
            "saveFilesDirectory": os.path.join(d, "out"), "savePlotsDirectory": os.path.join(d, "plots")}


def rewrite_config(configFile, values):
    """The text of ``configFile`` with the value of every ``key = value`` line whose key is in ``values`` replaced; all
    other lines, comments and line ends stay as they are."""
    out = []
    with open(configFile, newline="") as fh:
        for raw in fh:
            body = raw.rstrip("\r\n")
            key = body.split(" = ")[0]
            if " = " in body and key in values and not body.startswith("#"):
                out.append(key + " = " + str(values[key]) + raw[len(body):])
            else:
                out.append(raw)
    return "".join(out)


def scaffold_counts(coarseBins):
    """(scaffolds, scaffolds of one bin) of a bin list whose scaffolds are contiguous."""
    per = {}
    for b in coarseBins:
        per[b.chrom] = per.get(b.chrom, 0) + 1
    return len(per), sum(1 for c in per.values() if c == 1)


def write_resolution(ctx, binList, paths, configFile, v, ice, balance, line):
    """The file set of one resolution from the context that owns its raw map (shared with buildMap): the bed file, the
    raw ``.matrix``, unless ``balance`` is off the ``_iced.matrix`` and its ``.biases`` (iceNormalize.balanceResident with
    the config's ``ice*`` settings; the context's matrix becomes the balanced map) and ``config.txt``.  ``line``: the start
    of the line printed for it.  Returns (the five ICE columns of the summary, read pairs)."""
    from . import iceNormalize
    for d in (paths["dir"], paths["saveFilesDirectory"], paths["savePlotsDirectory"]):
        os.makedirs(d, exist_ok=True)
    ids = [b.ID for b in binList]
    res = int(paths["resolution"])
    counts = ctx.contacts_host()
    pairs = float(np.triu(counts).sum())
    write_bed(paths["hicProBedFile"], binList)
    write_iced_matrix(paths["hicProRawMatrixFile"], counts, ids)
    del counts
    line += ", read pairs %r" % pairs
    ice_cols = ["NA"] * 5
    if balance:
        short = None
        if ice["iceMinScaffoldSize"] is not None:
            short = iceNormalize.short_scaffold_bins(binList, v["hicProScaffSizeFile"], ice["iceMinScaffoldSize"])
        mask, (n_a, n_b, n_c), bias, iters, delta = iceNormalize.balanceResident(
            ctx, short, ice["iceFilterLowPerc"], ice["iceMaxIter"], ice["iceEps"])
        write_biases(paths["hicProBiasFile"], bias)
        write_iced_matrix(paths["hicProMatrixFile"], ctx.contacts_host(), ids)
        line += ", masked %d (scaffold size %d, no counts %d, low counts %d), iterations %d, final delta %r" % (
            int(mask.sum()), n_a, n_b, n_c, iters, delta)
        ice_cols = [str(n_a), str(n_b), str(n_c), str(iters), repr(delta)]
        if iters >= ice["iceMaxIter"] and not delta < ice["iceEps"]:
            print("WARNING... ICE did not converge in iceMaxIter = %d iterations at resolution %d (delta %r >= "
                  "iceEps %r); the map of the last iteration is written" % (ice["iceMaxIter"], res, delta, ice["iceEps"]))
    text = rewrite_config(configFile, {key: paths[key] for key in REWRITTEN_KEYS})
    # a key the input config leaves out (buildMap needs no hicProRawMatrixFile) is added at the end
    missing = [key for key in REWRITTEN_KEYS if key not in v or v[key] == ""]
    if missing:
        text += ("" if text.endswith("\n") or not text else "\n") + "".join("%s = %s\n" % (key, paths[key]) for key in missing)
    with open(os.path.join(paths["dir"], "config.txt"), "w", newline="") as fh:
        fh.write(text)
    print(line)
    return ice_cols, pairs


def runPipeline(configFile, factors, outDir=None, balance=True, device=0):
    from . import run_hicAssembler as driver
    v = driver.readConfigFileToVariables(configFile)
    raw, ice = driver.part0Settings(v)
    if not isinstance(v["resolution"], int):
        sys.exit("ERROR... resolution must be set in the config file. Exiting...")
    if outDir is None:
        outDir = os.path.join(v["saveFilesDirectory"], "rebin")
    with paused_gc():
        binList = read_bed_bins(v["hicProBedFile"])
        try:
            plans = [(k,) + rebin_bins(binList, k) for k in factors]
        except ValueError as exc:
            sys.exit("ERROR... %s: the bins of a scaffold are merged from its own start. Exiting..." % exc)
        host = read_contact_matrix(raw, binList)
        rows = []
        with _lib.Context(device) as fine:
            fine.set_contacts(host)
            del host
            ptr, n, ld = fine.contacts_device()
            for k, coarse, group_start in plans:
                res = k * v["resolution"]
                paths = output_paths(outDir, res)
                n_scaf, n_one = scaffold_counts(coarse)
                with _lib.Context(device) as ctx:
                    ctx.set_contacts_device(ptr, n, ld, keepalive=fine)
                    ctx.rebin(group_start)
                    line = "REBIN: factor %d, resolution %d, bins %d (scaffolds %d, of one bin %d)" % (
                        k, res, len(coarse), n_scaf, n_one)
                    ice_cols, pairs = write_resolution(ctx, coarse, paths, configFile, v, ice, balance, line)
                rows.append([str(k), str(res), str(len(coarse)), str(n_scaf), str(n_one)] + ice_cols + [repr(pairs)])
    with open(os.path.join(os.path.abspath(outDir), "rebin_summary.tsv"), "w") as fh:
        fh.write("#" + "\t".join(SUMMARY_COLUMNS) + "\n")
        fh.write("".join("\t".join(r) + "\n" for r in rows))
    return rows


def main(argv=None):
    parser = argparse.ArgumentParser(description="Sums the raw HiC-Pro map (hicProRawMatrixFile) to coarser resolutions on the "
                                                 "GPU and balances each, ready for -part1 -part2.")
    parser.add_argument("-config", help="Full file path to the config file", required=True, type=str)
    parser.add_argument("-factor", help="Comma-separated factors k (2 .. 64): one output per resolution k * resolution",
                        required=True, type=str)
    parser.add_argument("-out", help="Output directory (default: saveFilesDirectory/rebin)", type=str, default=None)
    parser.add_argument("-noBalance", help="Write the bed file and the raw map only, no ICE", action="store_true")
    parser.add_argument("-device", help="GPU index (default 0)", type=int, default=0)
    args = parser.parse_args(argv)
    try:
        factors = parse_factors(args.factor)
    except ValueError as exc:
        sys.exit("ERROR... %s. Exiting..." % exc)
    runPipeline(args.config, factors, args.out, balance=not args.noBalance, device=args.device)


if __name__ == "__main__":
    main()
