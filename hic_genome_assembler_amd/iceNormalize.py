"""Part 0: ICE balancing of a raw HiC-Pro map on the device.

HiC-Pro's ``ice`` step (``ice --filter_low_counts_perc 0.02 --filter_high_counts_perc 0 --max_iter 100 --eps 0.1
--remove-all-zeros-loci --output-bias 1``) turns the raw triplet file into the ``*_iced.matrix`` / ``*.biases`` pair that
Parts 1 and 2 (and the reference) start from.  The reference's README asks for scaffolds under about 10 kb to be dropped
BEFORE that normalisation; with the raw map resident on the GPU both are one call here:

* the mask is built on the host (:func:`build_mask`): (a) bins of scaffolds shorter than ``minScaffoldSize`` bp,
  (b) bins without a read, (c) the ``filterLowPerc`` bins with the fewest reads;
* the iteration runs on the device (``hicmi_ice_balance``: one read-only pass over the raw map per iteration);
* the balanced map and the biases are written in the files the loaders read, ``nan`` biases for the masked bins - which
  ``initiateLoci`` drops, so they leave the pipeline without a code path of their own.

``python -m hic_genome_assembler_amd.iceNormalize -config FILE [-device 0]`` runs it alone; ``run_hicAssembler.py -part0``
runs it in front of the other parts.
"""
from __future__ import annotations

import argparse
import time

import numpy as np

from . import _lib
from .hostio import paused_gc, read_bed_bins, read_contact_matrix, write_biases, write_iced_matrix


def short_scaffold_bins(binList, scaffSizeFile, minScaffoldSize):
    """Rule (a): True for every bin whose scaffold is shorter than ``minScaffoldSize`` bp in the size file
    (``name<TAB>size`` lines, as Part 1's assessment reads them)."""
    sizes = {}
    with open(scaffSizeFile) as fh:
        for line in fh:
            cols = line.strip("\r").strip("\n").split("\t")
            if len(cols) >= 2:
                sizes[cols[0]] = int(cols[1])
    missing = sorted({b.chrom for b in binList} - set(sizes))
    if missing:
        raise ValueError("iceMinScaffoldSize is set but hicProScaffSizeFile has no size for %d scaffold(s), e.g. %s"
                         % (len(missing), missing[0]))
    return np.fromiter((sizes[b.chrom] < minScaffoldSize for b in binList), dtype=bool, count=len(binList))


def build_mask(weights, short_bins=None, filterLowPerc=0.02):
    """Rules (b) and (c) on the row weights ``w_i = sum_j C_ij`` of the map after rule (a) (``short_bins``: its mask, or
    None).  (b) masks the bins with w == 0; (c), for p = filterLowPerc > 0, those with w < x[int(n p)], x = w sorted
    ascending over all n bins (bins equal to the threshold stay).  Returns (mask, masked by (a), by (b), by (c)), each
    bin counted under the first rule that takes it."""
    w = np.asarray(weights, dtype=np.float64)
    n = len(w)
    mask = np.zeros(n, dtype=bool) if short_bins is None else np.array(short_bins, dtype=bool)
    n_a = int(mask.sum())
    mask |= w == 0
    n_b = int(mask.sum()) - n_a
    if filterLowPerc > 0 and n:
        mask |= w < np.sort(w)[int(n * filterLowPerc)]
    n_c = int(mask.sum()) - n_a - n_b
    return mask, n_a, n_b, n_c


def balanceResident(ctx, short_bins=None, filterLowPerc=0.02, maxIter=100, eps=0.1):
    """The device part on a context that owns the raw map: returns (mask, (masked by (a), (b), (c)), biases with nan for
    the masked bins, iterations, final delta).  The context's matrix becomes the balanced map."""
    if short_bins is not None and short_bins.any():
        ctx.ice_mask_rows(short_bins)
    weights, _seq = ctx.row_sums()
    mask, n_a, n_b, n_c = build_mask(weights, short_bins, filterLowPerc)
    bias, iters, delta = ctx.ice_balance(mask, maxIter, eps)
    return mask, (n_a, n_b, n_c), bias, iters, delta


def runPipeline(bedFile, rawMatrixFile, scaffSizeFile, matrixFile, biasFile, filterLowPerc=0.02, maxIter=100, eps=0.1,
                minScaffoldSize=None, device=0, keep_resident=False):
    """Raw counts in, balanced map and biases out.  ``keep_resident=True``: the context, its matrix compacted to the
    unmasked bins (the bins initiateLoci will read from the two files just written), is returned for Part 1 of the same
    run instead of being closed."""
    print("########################################")
    print("### Working on Part0 of the pipeline ###")
    t_all = time.time()
    with paused_gc():
        binList = read_bed_bins(bedFile)
        n = len(binList)
        short = short_scaffold_bins(binList, scaffSizeFile, minScaffoldSize) if minScaffoldSize is not None else None
        host = read_contact_matrix(rawMatrixFile, binList)
        ctx = _lib.Context(device)
        try:
            ctx.set_contacts(host)
            del host
            mask, (n_a, n_b, n_c), bias, iters, delta = balanceResident(ctx, short, filterLowPerc, maxIter, eps)
            print("ICE: bins %d, masked %d (scaffold size %d, no counts %d, low counts %d), iterations %d, final delta %r"
                  % (n, int(mask.sum()), n_a, n_b, n_c, iters, delta))
            if iters >= maxIter and not delta < eps:
                print("WARNING... ICE did not converge in iceMaxIter = %d iterations (delta %r >= iceEps %r); the map of "
                      "the last iteration is written" % (maxIter, delta, eps))
            write_biases(biasFile, bias)
            write_iced_matrix(matrixFile, ctx.contacts_host(), [b.ID for b in binList])
            if keep_resident and mask.any():
                if mask.all():
                    raise ValueError("ICE masked every bin: nothing is left for Part 1")
                ctx.compact(np.flatnonzero(~mask))
        except BaseException:
            ctx.close()
            raise
    print("Total run-time of Part0 = " + str(time.time() - t_all))
    print("- Part 0 (ICE balancing of the raw map) completed successfully")
    if keep_resident:
        return ctx
    ctx.close()
    return None


def main(argv=None):
    from . import run_hicAssembler as driver
    parser = argparse.ArgumentParser(description="ICE-balances the raw HiC-Pro map (hicProRawMatrixFile) on the GPU.")
    parser.add_argument("-config", help="Full file path to the config file", required=True, type=str)
    parser.add_argument("-device", help="GPU index (default 0)", type=int, default=0)
    args = parser.parse_args(argv)
    v = driver.readConfigFileToVariables(args.config)
    raw, ice = driver.part0Settings(v)
    runPipeline(v["hicProBedFile"], raw, v["hicProScaffSizeFile"], v["hicProMatrixFile"], v["hicProBiasFile"],
                ice["iceFilterLowPerc"], ice["iceMaxIter"], ice["iceEps"], ice["iceMinScaffoldSize"], device=args.device)


if __name__ == "__main__":
    main()
