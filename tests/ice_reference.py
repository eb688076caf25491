"""NumPy restatement of the ICE definition (HiC-Pro's ``ice --filter_low_counts_perc 0.02
--filter_high_counts_perc 0 --max_iter 100 --eps 0.1 --remove-all-zeros-loci --output-bias 1``), written from the
definition alone: the literal in-place loop on a copy of the matrix.  It shares no code with the package - the GPU tests
compare the device against it, the CPU tests check its own sanity - and also builds the maps those tests run on.
"""
from __future__ import annotations

import numpy as np


def ice_mask(counts, short_bins=None, filter_low_perc=0.02):
    """Rules (a)-(c): returns (mask, number of bins masked by (a), by (b), by (c)).  ``short_bins``: boolean per bin, True
    where the bin's scaffold is shorter than iceMinScaffoldSize (None: the key is not set)."""
    c = np.array(counts, dtype=np.float64)
    n = c.shape[0]
    mask = np.zeros(n, dtype=bool)
    if short_bins is not None:
        mask |= np.asarray(short_bins, dtype=bool)
        c[mask, :] = 0.0
        c[:, mask] = 0.0
    n_a = int(mask.sum())
    w = c.sum(axis=1)
    mask |= w == 0
    n_b = int(mask.sum()) - n_a
    if filter_low_perc > 0:
        x = np.sort(w)
        mask |= w < x[int(n * filter_low_perc)]
    n_c = int(mask.sum()) - n_a - n_b
    return mask, n_a, n_b, n_c


def ice_balance(counts, mask, max_iter=100, eps=0.1):
    """The loop: returns (X, bias with nan for masked bins, iterations run, last sum |bias_prev - bias| or nan, and the
    list of every sum |bias_prev - bias| the stop test looked at, iterations 1, 2, ...)."""
    X = np.array(counts, dtype=np.float64)
    n = X.shape[0]
    mask = np.asarray(mask, dtype=bool)
    X[mask, :] = 0.0
    X[:, mask] = 0.0
    bias = np.ones(n)
    mean0 = X.sum() / n ** 2
    bias_prev = None
    delta, deltas, iters = float("nan"), [], 0
    for it in range(max_iter):
        s = X.sum(axis=1)
        nz = s != 0
        d = np.ones(n)
        d[nz] = s[nz] / s[nz].mean()
        bias *= d
        X /= d[:, None] * d[None, :]
        c = (X.sum() / n ** 2) / mean0
        bias *= np.sqrt(c)
        X /= c
        iters = it + 1
        if it > 0:
            delta = float(np.abs(bias_prev - bias).sum())
            deltas.append(delta)
            if delta < eps:
                break
        bias_prev = bias.copy()
    out = bias.copy()
    out[mask] = np.nan
    return X, out, iters, delta, deltas


def stop_margin(deltas, eps):
    """min over the iterations of | sum |bias_prev - bias| - eps | / eps: how far the stop decision ever was from
    hinging on rounding (inf when no test was made)."""
    return min((abs(d - eps) / eps for d in deltas), default=float("inf"))


# ---- the maps of tests/test_gpu_ice.py ------------------------------------------------------------------------------
RESOLUTION = 100000
MIN_SCAFFOLD_SIZE = 10000          # iceMinScaffoldSize of the n = 257 case; its two short scaffolds have 5,000 bp
SIZES = [2, 5, 63, 64, 65, 257, 1000]
SETTINGS = [(0.1, 100), (1e-6, 100), (1e-12, 7)]


def make_case(n, seed=1):
    """(raw counts, layout, short_bins or None) of the n-bin test map: block-diagonal 1 / (1 + d) decay times log-normal
    per-bin factors (sigma 0.5), Poisson counts; one dead bin from n = 63 on; two scaffolds under MIN_SCAFFOLD_SIZE at
    n = 257."""
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(n, seed=seed, n_chrom=1 if n < 63 else (2 if n < 257 else 3), mean_scaffold_bins=6.0,
                            resolution=RESOLUTION)
    dead = (n // 3,) if n >= 63 else ()
    counts, lay = synth.make_raw_counts(lay, seed=seed, dead_bins=dead, short_scaffolds=2 if n == 257 else 0,
                                        short_size_bp=MIN_SCAFFOLD_SIZE // 2)
    short = None
    if n == 257:
        short = lay.scaffold_sizes_bp[lay.scaffold_of_bin] < MIN_SCAFFOLD_SIZE
    return counts, lay, short
