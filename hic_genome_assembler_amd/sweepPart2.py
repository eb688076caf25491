"""Part 2 parameter sweep: one map, one GPU, many ``nScaffolds x scanScaffolds`` settings.

    python -m hic_genome_assembler_amd.sweepPart2 -config cfg.txt -nScaffolds 5,6,7,8 -scanScaffolds 4,5,6,7,8
           [-chromosomeGroupFile FILE] [-device 0] [-out DIR] [-plots] [-support]

The map is read once (the grouped bins only, as ``-part2`` reads it).  The settings are the distinct pairs after
orderGenome._startChromosome's clamps (nScaffolds >= 9 -> 8, scanScaffolds > nScaffolds -> nScaffolds).  Chromosomes are ordered
independently (OG:608-612), and per chromosome of S scaffolds the work is shared between settings:

* S <= nScaffolds: brute force over all S scaffolds, the do-while re-insertion of the last one (OG:475-493), no scan -
  one job for every such setting;
* S > nScaffolds: selection, brute force and insertion depend on nScaffolds alone, only the scan on scanScaffolds.

The jobs go through the one Part 2 driver, orderGenome.orderJobs, which a ``-part2`` run uses for its one-setting grid:
one lane (context and layout) per (chromosome, brute-force width); every start phase in one hicmi_p2_start_all call; all
insertion loops in one hicmi_p2_insert_all_multi lock step; the scans on a pool of HICMI_PART2_WORKERS threads, entered
through hicmi_p2_scan_arranged, each on its own copy of the insertion result.  Contexts without those entry points run
the same steps one after the other on the one context.  What is left here is the plan, each job's printed lines, and
final_score.

``DIR/nScaffolds<a>_scanScaffolds<b>/`` holds the chromosomeOrderFile and plotOrderFile (config base names) that
``-part2`` writes with that setting and ``part2.log`` with the lines a one-worker ``-part2`` run prints from "Chromosomes
found" to the last "Final ordering" block.  ``DIR/sweep_summary.tsv`` has one row per setting,
``DIR/chromosome_scores.tsv`` one row per chromosome, and ``DIR/best/`` the two files with each chromosome ordered by the
setting of its highest final_score (ties: the earlier setting in grid order).  final_score is the literal objective
(hicmi_p2_score_exact, NumPy-trace order) of a chromosome's final bin order under ONE total per chromosome, the total
of its selection (what hicmi_p2_total returns for it), so that settings compare on one footing; it is not the printed
bestCost, whose total is rounded in arrangement order (OG:343 vs OG:506).  DIR defaults to saveFilesDirectory/sweep_part2.
``-support`` also writes ``DIR/best/placementSupport.txt``, the placement-support report (orderGenome.placementSupport) of
the best orderings; its score0 column is their final_score - and ``DIR/best/breakSupport.txt``, their break-support
report (orderGenome.breakSupport).
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import threading
import time

import numpy as np

from . import orderGenome as p2
from . import plotContactMaps as plotModule
from .hostio import initiateLoci, paused_gc
from .run_hicAssembler import ensureAllVariablesAreSet, readConfigFileToVariables
from .sweepPart1 import parse_values

SUMMARY_COLUMNS = ["nScaffolds", "scanScaffolds", "chromosomes", "chromosomes_scanned", "scan_rounds", "best_for",
                   "final_scores"]


def clamp(nScaffolds, scanScaffolds):
    """_startChromosome's clamps (orderGenome.py, OG:551-556)."""
    nScaffolds = 8 if nScaffolds >= 9 else nScaffolds
    return nScaffolds, min(scanScaffolds, nScaffolds)


def settings(nScaffolds, scanScaffolds):
    """The distinct clamped (nScaffolds, scanScaffolds) pairs in grid order (nScaffolds, then scanScaffolds), and
    {setting: requested pairs} for the settings more than one requested pair folded into."""
    out, folded = [], {}
    for a in nScaffolds:
        for b in scanScaffolds:
            s = clamp(int(a), int(b))
            if s not in out:
                out.append(s)
            folded.setdefault(s, []).append((int(a), int(b)))
    return out, {s: v for s, v in folded.items() if len(v) > 1}


def setting_name(nScaffolds, scanScaffolds):
    return "nScaffolds%d_scanScaffolds%d" % (nScaffolds, scanScaffolds)


def start_key(c, S, nScaffolds):
    """What selection, brute force and insertion of chromosome c (S scaffolds) depend on."""
    return (c, min(S, nScaffolds))


def scan_key(c, S, nScaffolds, scanScaffolds):
    """What the final order of chromosome c depends on: no scan when S <= nScaffolds."""
    return (c, S, None) if S <= nScaffolds else (c, nScaffolds, scanScaffolds)


def plan(scaffold_counts, grid):
    """The shared jobs of a sweep: {start key: None} and {scan key: start key} in first-use order, and per setting the
    scan key of every chromosome."""
    starts, scans, per_setting = {}, {}, []
    for nS, sc in grid:
        keys = []
        for c, S in enumerate(scaffold_counts):
            sk, fk = start_key(c, S, nS), scan_key(c, S, nS, sc)
            starts.setdefault(sk, None)
            scans.setdefault(fk, sk)
            keys.append(fk)
        per_setting.append(keys)
    return starts, scans, per_setting


def best_settings(scores):
    """scores[setting][chromosome] -> per chromosome the index of the setting with the highest score (the first one in
    grid order on a tie)."""
    n_chrom = len(scores[0]) if scores else 0
    out = []
    for c in range(n_chrom):
        best = 0
        for s in range(1, len(scores)):
            if scores[s][c] > scores[best][c]:
                best = s
        out.append(best)
    return out


def _is_runtime_line(line):
    return "time = " in line or line.startswith("Total run-time") or line.startswith("RunTime")


class _ThreadOut(io.TextIOBase):
    """sys.stdout for the scan pool: what a thread prints goes to its own buffer while it has one."""

    def __init__(self, real):
        self.real = real
        self.local = threading.local()

    def write(self, s):
        buf = getattr(self.local, "buf", None)
        return (buf if buf is not None else self.real).write(s)

    def flush(self):
        self.real.flush()


def _lines(fn, *args, **kw):
    """fn's result and the lines it printed (on this thread)."""
    out = sys.stdout
    if isinstance(out, _ThreadOut):
        prev = getattr(out.local, "buf", None)
        out.local.buf = io.StringIO()
        try:
            res = fn(*args, **kw)
            text = out.local.buf.getvalue()
        finally:
            out.local.buf = prev
        return res, text.splitlines()
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = fn(*args, **kw)
    return res, buf.getvalue().splitlines()


def _final_scores(started, finished, start_of_scan, chromosome_of):
    """final_score of every scan job: the literal objective of its final bin order under ONE total per chromosome, that of
    the chromosome's whole selection.  One hicmi_p2_score_exact call per start job, over the distinct final orders of its
    scans that no earlier job of the chromosome ended with."""
    totals, cache, key_of = {}, {}, [None] * len(finished)
    scans_of = [[] for _ in started]
    for s, j in enumerate(start_of_scan):
        scans_of[j].append(s)
    for (lane, layout, _lines), c, mine in zip(started, chromosome_of, scans_of):
        lane.select(layout)                              # (a context without worker lanes has served other layouts since)
        if c not in totals:
            totals[c] = layout.whole_total()
        rows = {}
        for s in mine:
            ids, rev = layout.describe(finished[s][0][0])
            key_of[s] = (c, ids.tobytes() + rev.tobytes())
            if key_of[s] not in cache:
                rows[key_of[s]] = layout.node_row(ids, rev)
        if rows:
            vals = [0.0] * len(rows) if layout.n < 2 else \
                lane.ctx.p2_score_exact(np.stack(list(rows.values())).astype(np.int32), totals[c])
            cache.update(zip(rows, map(float, vals)))
    return [cache[k] for k in key_of]


def order_settings(matrix, chromList, binList, grid, workers=None, report=print):
    """Every chromosome of ``chromList`` ordered at every (nScaffolds, scanScaffolds) of ``grid`` (clamped pairs) with
    the work shared as the module docstring says.  Returns a dict with, per setting, per chromosome: 'orders' (scaffold
    lists), 'lines' (what a one-worker -part2 run prints for it), 'scores' (final_score), 'rounds', 'scanned'; and
    'counts' (jobs requested / run)."""
    counts = [len({name for _b, name in chrom}) for chrom in chromList]
    starts, scans, per_setting = plan(counts, grid)
    n_jobs = len(grid) * len(chromList)
    report("- Part 2 sweep plan: %d settings x %d chromosomes = %d orderings; brute force + insertion jobs: %d requested / "
           "%d run; scan jobs: %d requested / %d run" % (len(grid), len(chromList), n_jobs, n_jobs, len(starts), n_jobs,
                                                         len(scans)))
    start_keys, scan_keys = list(starts), list(scans)
    start_of_scan = [start_keys.index(scans[fk]) for fk in scan_keys]
    t0 = time.time()
    real = sys.stdout
    sys.stdout = _ThreadOut(real)                        # the scan threads' lines, job by job (_lines)
    try:
        started, finished = p2.orderJobs(matrix, chromList, binList, start_keys,
                                         [(j, fk[2]) for j, fk in zip(start_of_scan, scan_keys)],
                                         p2.WORKERS if workers is None else workers, capture=_lines)
    finally:
        sys.stdout = real
    scores = _final_scores(started, finished, start_of_scan, [sk[0] for sk in start_keys])
    report("- Part 2 sweep: %d brute-force / insertion jobs and %d scans in %.3f s" % (len(starts), len(scans),
                                                                                      time.time() - t0))
    out = {"orders": [], "lines": [], "scores": [], "rounds": [], "scanned": [], "text": [],
           "counts": {"orderings": n_jobs, "start_jobs": len(starts), "scan_jobs": len(scans)},
           "start_keys": start_keys, "scan_keys": scan_keys}
    scan_index = {fk: s for s, fk in enumerate(scan_keys)}
    for keys in per_setting:
        o, ln, sc, rd, sd, tx = [], [], [], [], [], []
        for fk in keys:
            s = scan_index[fk]
            (res, text), lines = finished[s]
            o.append(res)
            ln.append([*started[start_of_scan[s]][2], *lines])
            sc.append(scores[s])
            rd.append(sum(1 for line in lines if line.startswith("Working on round ")))
            sd.append(fk[2] is not None)
            tx.append(text)
        for k, v in zip(("orders", "lines", "scores", "rounds", "scanned", "text"), (o, ln, sc, rd, sd, tx)):
            out[k].append(v)
    return out


def _write_files(d, orders, text, chromosomeOrderFile, plotOrderFile):
    os.makedirs(d, exist_ok=True)
    _lines(p2.writeScaffoldOrderingsToFile, orders, os.path.join(d, os.path.basename(chromosomeOrderFile)),
           [t[0] for t in text])
    _lines(p2.writeBinIDsOrderingToFile, [s for g in orders for s in g], os.path.join(d, os.path.basename(plotOrderFile)),
           [t[1] for t in text])


def write_summary(outDir, grid, res, chromList, best):
    with open(os.path.join(outDir, "sweep_summary.tsv"), "w") as fh:
        fh.write("\t".join(SUMMARY_COLUMNS) + "\n")
        for s, (nS, sc) in enumerate(grid):
            fh.write("\t".join([str(nS), str(sc), str(len(chromList)), str(sum(res["scanned"][s])),
                                str(sum(res["rounds"][s])), str(sum(1 for b in best if b == s)),
                                ",".join(repr(v) for v in res["scores"][s])]) + "\n")
    with open(os.path.join(outDir, "chromosome_scores.tsv"), "w") as fh:
        fh.write("\t".join(["chromosome", "bins", "scaffolds"] + [setting_name(*g) for g in grid] + ["best"]) + "\n")
        for c, chrom in enumerate(chromList):
            fh.write("\t".join([str(c + 1), str(len(chrom)), str(len({nm for _b, nm in chrom}))]
                               + [repr(res["scores"][s][c]) for s in range(len(grid))] + [setting_name(*grid[best[c]])])
                     + "\n")


def read_summary(path):
    """sweep_summary.tsv back as rows of strings, final_scores as a list of floats."""
    with open(path) as fh:
        head = fh.readline().rstrip("\n").split("\t")
        rows = []
        for line in fh:
            r = dict(zip(head, line.rstrip("\n").split("\t")))
            r["final_scores"] = [float(v) for v in r["final_scores"].split(",") if v]
            rows.append(r)
    return rows


def _plots(matrix, binList, orders, outDir, fullGenomePlot, fullGenomePlotTitle, resolution, suffix):
    where = matrix.bin_index(binList)
    for i, group in enumerate(orders):
        rows = [where[b] for s in group for b in s.binList]
        if rows:
            plotModule.plotContactMap(plotModule.DeviceImage(matrix.ctx, 0, rows), resolution=resolution, tickCount=11,
                                      highlightChroms=False, wInches=24, hInches=24, lP=1, hP=98, reverseColorMap='',
                                      showPlot=False, savePlot=os.path.join(outDir, "Chr_%d.png" % (i + 1)),
                                      title="Chr_%d" % (i + 1), titleSuffix=suffix)
    rows = [where[b] for group in orders for s in group for b in s.binList]
    plotModule.plotContactMap(plotModule.DeviceImage(matrix.ctx, 0, rows), resolution=resolution, tickCount=11,
                              highlightChroms=p2.getChromosomeOutlineCoords(orders), wInches=32, hInches=32, lP=2, hP=98,
                              reverseColorMap='', showPlot=False,
                              savePlot=os.path.join(outDir, os.path.basename(fullGenomePlot)), title=fullGenomePlotTitle,
                              titleSuffix=False)


def runSweep(hicProBedFile, hicProBiasFile, hicProMatrixFile, chromosomeGroupFile, chromosomeOrderFile, plotOrderFile,
             nScaffolds, scanScaffolds, outDir, resolution=100000, plots=False, fullGenomePlot="fullGenome.png",
             fullGenomePlotTitle="", chromosomePlotSuffix=False, device=0, shard=None, support=False):
    """OG:679-712 for every setting of the grid on one map (see the module docstring).  Returns a dict: 'grid' (the
    clamped settings), 'folded', 'best' (per chromosome the index of its best setting) and order_settings' results."""
    if shard is not None and shard[1] > 1:
        raise ValueError("a Part 2 sweep runs on one GPU: row shards (one map over several GPUs) are not supported")
    grid, folded = settings(nScaffolds, scanScaffolds)
    os.makedirs(outDir, exist_ok=True)
    print("### Part 2 sweep: %d settings ###" % len(grid))
    for s, pairs in folded.items():
        print("- nScaffolds/scanScaffolds %s are the same setting after the clamps: %s"
              % (", ".join("%d/%d" % p for p in pairs), setting_name(*s)))
    t_all = time.time()
    binDict = p2.readGroupingsToValidBins(chromosomeGroupFile)
    binList = initiateLoci(hicProBedFile, hicProBiasFile, binID_dict=binDict)
    matrix = p2.buildAdjacencyMatrix(hicProMatrixFile, binList, device=device)
    try:
        with paused_gc():
            chromList, head = _lines(p2.readChromsFromFile, chromosomeGroupFile)
            res = order_settings(matrix, chromList, binList, grid)
            best = best_settings(res["scores"])
            for s, g in enumerate(grid):
                d = os.path.join(outDir, setting_name(*g))
                _write_files(d, res["orders"][s], res["text"][s], chromosomeOrderFile, plotOrderFile)
                log = list(head) + [ln for c in range(len(chromList)) for ln in res["lines"][s][c]]
                with open(os.path.join(d, "part2.log"), "w") as fh:
                    fh.write("\n".join(ln for ln in log if not _is_runtime_line(ln)) + "\n")
            best_orders = [res["orders"][best[c]][c] for c in range(len(chromList))]
            best_text = [res["text"][best[c]][c] for c in range(len(chromList))]
            _write_files(os.path.join(outDir, "best"), best_orders, best_text, chromosomeOrderFile, plotOrderFile)
            write_summary(outDir, grid, res, chromList, best)
            if support:
                _lines(p2.writePlacementSupportToFile, p2.placementSupport(matrix, best_orders, binList, chromList),
                       os.path.join(outDir, "best", "placementSupport.txt"))
                _lines(p2.writeBreakSupportToFile, p2.breakSupport(matrix, best_orders, binList, chromList),
                       os.path.join(outDir, "best", "breakSupport.txt"))
            if plots and plotModule.plots_enabled(fullGenomePlot):
                _plots(matrix, binList, best_orders, os.path.join(outDir, "best"), fullGenomePlot, fullGenomePlotTitle,
                       resolution, chromosomePlotSuffix)
    finally:
        matrix.ctx.close()
    print("Total run-time of the Part 2 sweep = " + str(time.time() - t_all))
    return dict(res, grid=grid, folded=folded, best=best)


def _parse_args(argv):
    p = argparse.ArgumentParser(description="Part 2 parameter sweep on one map and one GPU: every nScaffolds x "
                                            "scanScaffolds setting, with the brute force, insertion and scan work "
                                            "shared between settings where it is the same.")
    p.add_argument("-config", required=True, type=str, help="run_hicAssembler.py config file")
    p.add_argument("-nScaffolds", type=str, help="comma-separated values (default: the config's)")
    p.add_argument("-scanScaffolds", type=str, help="comma-separated values (default: the config's)")
    p.add_argument("-chromosomeGroupFile", type=str, default=None,
                   help="group file to order (default: the config's), e.g. one written by a Part 1 sweep")
    p.add_argument("-device", type=int, default=0, help="GPU index (default 0)")
    p.add_argument("-out", type=str, default=None, help="output directory (default: saveFilesDirectory/sweep_part2)")
    p.add_argument("-plots", action="store_true", help="draw the best orderings' chromosome and genome figures")
    p.add_argument("-support", action="store_true", help="write the placement-support and break-support reports of the best orderings")
    return p.parse_args(argv)


def grid_from_args(args, v):
    """The two value lists of the command line, each defaulting to the config's single value."""
    return tuple(parse_values(getattr(args, key), key, v[key]) if getattr(args, key) is not None else [v[key]]
                 for key in ("nScaffolds", "scanScaffolds"))


def main(argv=None):
    args = _parse_args(argv)
    v = readConfigFileToVariables(args.config)
    if ensureAllVariablesAreSet(v):
        sys.exit(2)
    nScaffolds, scanScaffolds = grid_from_args(args, v)
    out = args.out or os.path.join(v["saveFilesDirectory"], "sweep_part2")
    runSweep(v["hicProBedFile"], v["hicProBiasFile"], v["hicProMatrixFile"],
             args.chromosomeGroupFile or v["chromosomeGroupFile"], v["chromosomeOrderFile"], v["plotOrderFile"],
             nScaffolds, scanScaffolds, out, resolution=v["resolution"], plots=args.plots,
             fullGenomePlot=v["fullGenomePlot"], fullGenomePlotTitle=v["fullGenomePlotTitle"],
             chromosomePlotSuffix=v["chromosomePlotSuffix"], device=args.device, support=args.support)


if __name__ == "__main__":
    main()
