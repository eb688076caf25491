"""Part 1 parameter sweep: one map, one GPU, many ``minSize x psig x modularity (x louvainRounds)`` settings.

    python -m hic_genome_assembler_amd.sweepPart1 -config cfg.txt -minSize 5,8,10,15 -psig .05,.01 -modularity 0,.05
           [-louvainRounds 20] [-device 0] [-out DIR] [-plots]

The map is loaded, clustered (UPGMA) and ranked once - none of that depends on the three settings - and every
combination is then evaluated against the resident rank matrix: the two hypergeometric scan loops of all combinations run
in lock step on the device (hicmi_first_pass_cuts_multi / hicmi_filter_cuts_multi), the Louvain tail and the three group
files per combination.  Each combination's directory ``DIR/minSize<a>_psig<b>_modularity<c>[_louvainRounds<d>]/`` holds
the binGroupFile, assessmentFile and chromosomeGroupFile (config base names) that ``run_hicAssembler.py -part1`` with
that config writes, and ``part1.log`` with the lines such a run prints from the scan, Louvain and assessment stages
(run-time lines left out).  ``DIR/sweep_summary.tsv`` has one row per combination.  Any chromosomeGroupFile of the sweep
can be given to ``-part2``.  A flag that is not given takes the config's value; DIR defaults to saveFilesDirectory/sweep.
"""
from __future__ import annotations

import argparse
import collections
import contextlib
import io
import os
import sys
import time

from . import plotContactMaps as plotModule
from . import scaffoldToChromosomes as s2c
from .hostio import initiateLoci, paused_gc
from .run_hicAssembler import _convert, ensureAllVariablesAreSet, readConfigFileToVariables

SUMMARY_COLUMNS = ["minSize", "psig", "modularity", "louvainRounds", "first_pass_cuts", "filtered_cuts", "groups",
                   "louvain_groups", "scaffolds_assigned", "split_scaffolds", "cut_indices"]


def parse_values(text, key, config_value):
    """``"5,8,10"`` -> ``[5, 8, 10]``: every value is read with readConfigFileToVariables' rule for ``key`` (a bad
    value keeps the config's, with the parser's warning); repeated values are dropped, the order is kept."""
    out = []
    for item in str(text).split(","):
        item = item.strip()
        if not item:
            continue
        vals = {key: config_value}
        _convert(vals, key, item)
        if vals[key] not in out:
            out.append(vals[key])
    if not out:
        raise ValueError("-%s: no value given" % key)
    return out


def _fmt(v):
    return format(float(v), "g")


def combo_name(minSize, psig, modularity, louvainRounds=None):
    """The directory of one combination: minSize<a>_psig<b>_modularity<c>[_louvainRounds<d>]."""
    name = "minSize%d_psig%s_modularity%s" % (int(minSize), _fmt(psig), _fmt(modularity))
    return name if louvainRounds is None else name + "_louvainRounds%d" % int(louvainRounds)


def combinations(minSizes, psigs, modularities, louvainRounds):
    """The grid in the order the sweep runs it (minSize, then psig, then modularity, then louvainRounds)."""
    return [(a, b, c, d) for a in minSizes for b in psigs for c in modularities for d in louvainRounds]


def first_pass_key(n, minSize, modularity):
    """What the first pass of pre_process_all_matrix_breakpoints depends on: (min_size, stop_ind), or None when it
    returns [] before scanning (min_frac == 1)."""
    if modularity == 1:
        return None
    return (int(minSize), int(n - (n * modularity)))


def plan(n, combos):
    """The distinct scan loops of a grid: {first-pass key: modularity that gives it} (None not included) and, per
    combination, its first-pass key; the filter keys follow from the first-pass cuts."""
    fp = {}
    keys = []
    for ms, _ps, mod, _lr in combos:
        k = first_pass_key(n, ms, mod)
        keys.append(k)
        if k is not None and k not in fp:
            fp[k] = mod
    return fp, keys


def _captured(fn, *args, **kw):
    """fn's result and the lines it printed."""
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = fn(*args, **kw)
    return res, buf.getvalue().splitlines()


def _is_runtime_line(line):
    return "time = " in line or line.startswith("Total run-time") or line.startswith("Time to ")


def _multi_ok(ctx):
    return s2c._device_scan_loops(ctx) and hasattr(ctx, "first_pass_cuts_multi") and hasattr(ctx, "filter_cuts_multi")


def first_passes(rm, fp_keys):
    """{key: (cuts, printed lines)} for every first-pass key {(min_size, stop_ind): min_frac}: one lock-step call, or
    one pre_process_all_matrix_breakpoints per key when the context has no multi-set entry point."""
    res = {}
    ctx = rm.ctx
    multi = [k for k in fp_keys if k[0] >= 1]
    if multi and _multi_ok(ctx):
        for k, (cuts, mlog) in zip(multi, ctx.first_pass_cuts_multi(multi, .05)):      # the literal .05 (S2C:535)
            res[k] = (cuts, s2c.first_pass_report(cuts, mlog))
    for k, mod in fp_keys.items():
        if k not in res:
            res[k] = _captured(s2c.pre_process_all_matrix_breakpoints, rm, min_size=k[0], min_frac=mod, psig=.05)
    return res


def filters(rm, keys):
    """{(first-pass cuts, psig): (kept cuts, printed lines)}: one lock-step call, or one filter_noisy_breakpoints per
    key when the context has no multi-set entry point."""
    res = {}
    ctx = rm.ctx
    n = len(rm)
    multi = [k for k in keys if len(k[0]) and k[0][0] >= 0 and k[0][-1] < n
             and all(b > a for a, b in zip(k[0], k[0][1:]))]
    if multi and _multi_ok(ctx):
        for k, (out, warned) in zip(multi, ctx.filter_cuts_multi([list(k[0]) for k in multi], [k[1] for k in multi])):
            res[k] = (out, s2c.filter_report(list(k[0]), out, warned))
    for k in keys:
        if k not in res:
            res[k] = _captured(s2c.filter_noisy_breakpoints, rm, list(k[0]), psig=k[1])
    return res


def _split_scaffolds(binGroups):
    where = {}
    for g, grp in enumerate(binGroups):
        for _b, scaff in grp:
            where.setdefault(scaff, set()).add(g)
    return sum(1 for v in where.values() if len(v) > 1)


# ---- what both sweeps (this one and sweepHMM.py) share ----------------------------------------------------------------
Resident = collections.namedtuple("Resident", "adjMat binList prep writer")


@contextlib.contextmanager
def resident_map(hicProBedFile, hicProBiasFile, hicProMatrixFile, hicProScaffSizeFile, dendrogramOrderFile, device=0):
    """The map loaded, clustered (UPGMA) and reordered once, its dendrogramOrderFile queued on a writer thread: yields a
    Resident.  On the way out the writer is drained and the device context closed."""
    binList = initiateLoci(hicProBedFile, hicProBiasFile)
    adjMat = s2c.buildAdjacencyMatrix(hicProMatrixFile, binList, device=device)
    writer = s2c._FileWriter(True)
    try:
        with paused_gc():
            adjMat, binList, dendrogram, prep = s2c._cluster_resident(adjMat, binList, hicProScaffSizeFile,
                                                                      lambda _name: None, time.time())
            writer.submit(s2c.dendrogramLeafOrder_toFile, dendrogram, dendrogramOrderFile, prep["dend_lines"])
            yield Resident(adjMat, binList, prep, writer)
    finally:
        writer.finish()
        adjMat.ctx.close()


def write_setting(res, d, cuts, log, modularity, louvainRounds, is_runtime, files, plot=None, resolution=100000):
    """One setting's outputs in directory ``d``, from the cut indices of its boundary phase and the lines ``log`` that
    phase printed: the Louvain tail when modularity > 0 (its lines appended, run-time lines dropped by ``is_runtime``),
    the binGroupFile, assessmentFile and chromosomeGroupFile of ``files`` (their base names), part1.log and, when
    ``plot`` names a file, the outlined clustered map.  Returns the summary columns both sweeps have."""
    adjMat, binList, prep, writer = res
    n = adjMat.n
    binGroupFile, assessmentFile, chromosomeGroupFile = (os.path.join(d, os.path.basename(f)) for f in files)
    log = list(log)
    order, bins = list(adjMat.order), binList
    cuts_final = list(cuts)
    louvain_groups = 0
    with_louvain = modularity is not False and modularity > 0.0
    if with_louvain:
        start = sorted(cuts)[-1] if len(cuts) else 0
        if n - start > 0:
            (new_order, final), lines = _captured(s2c._louvain_tail, adjMat, binList, list(cuts), louvainRounds)
            log += [ln for ln in lines if not is_runtime(ln)]
            order = [order[i] for i in new_order]
            bins = [binList[i] for i in new_order]
            louvain_groups = len(final) + 1 - len(cuts)
            cuts_final = list(final)
    os.makedirs(d, exist_ok=True)
    writer.submit(s2c.writeBinGroupingsToFile, cuts_final, bins, binGroupFile, prep["bin_lines"])
    binGroups = s2c._bin_group_pairs(cuts_final, bins, prep["pairs"])
    log.append(str(len(binGroups)) + " chromosomes read in from file")
    chrGroups = s2c.assessChromosomeClustering(binGroups, assessmentFile, write=writer.submit,
                                               scaffolds=None if with_louvain else prep["scaffolds"])
    writer.submit(s2c.writeChromosomeGroupingsToFile, chrGroups, prep["sizes"], chromosomeGroupFile, prep["entry_lines"])
    writer.submit(s2c._write_text, os.path.join(d, "part1.log"), "\n".join(log) + "\n")
    if plot and plotModule.plots_enabled(plot):
        plotModule.plotContactMap(plotModule.DeviceImage(adjMat.ctx, 1, order), resolution=resolution,
                                  highlightChroms=cuts_final, showPlot=False,
                                  savePlot=os.path.join(d, os.path.basename(plot)))
    return {"groups": len(binGroups), "louvain_groups": louvain_groups,
            "scaffolds_assigned": sum(len(names) for names in chrGroups.scaffolds),
            "split_scaffolds": _split_scaffolds(binGroups), "cut_indices": cuts_final}


def write_summary(outDir, columns, rows):
    """``outDir/sweep_summary.tsv``: one row per setting, cut_indices comma-separated."""
    with open(os.path.join(outDir, "sweep_summary.tsv"), "w") as fh:
        fh.write("\t".join(columns) + "\n")
        for r in rows:
            fh.write("\t".join(",".join(str(c) for c in r[k]) if k == "cut_indices" else str(r[k])
                               for k in columns) + "\n")


# ------------------------------------------------------------------------------------------------
def runSweep(hicProBedFile, hicProBiasFile, hicProMatrixFile, hicProScaffSizeFile, dendrogramOrderFile,
             binGroupFile, assessmentFile, chromosomeGroupFile, minSizes, psigs, modularities, louvainRounds, outDir,
             name_louvain_rounds=None, avgClusterPlot_outlined=None, resolution=100000, plots=False, device=0,
             shard=None):
    """S2C:1117-1167 for every combination of the grid on one resident map (see the module docstring).  ``louvainRounds``:
    a list; ``name_louvain_rounds``: put it in the directory names (default: when it has more than one value).  Returns
    the summary rows (dicts keyed by SUMMARY_COLUMNS, cut_indices a list)."""
    if shard is not None and shard[1] > 1:
        raise ValueError("a Part 1 sweep runs on one GPU: row shards (one map over several GPUs) are not supported")
    if name_louvain_rounds is None:
        name_louvain_rounds = len(louvainRounds) > 1
    combos = combinations(minSizes, psigs, modularities, louvainRounds)
    os.makedirs(outDir, exist_ok=True)
    print("### Part 1 sweep: %d combinations ###" % len(combos))
    t_all = time.time()
    rows = []
    with resident_map(hicProBedFile, hicProBiasFile, hicProMatrixFile, hicProScaffSizeFile, dendrogramOrderFile,
                      device) as res:
        rm = s2c.rankOrderMatrix(res.adjMat)
        n = len(rm)
        t0 = time.time()
        fp_keys, combo_fp = plan(n, combos)
        fp = first_passes(rm, fp_keys)
        fp[None] = ([], [])                                   # min_frac == 1: no scan, nothing printed
        flt_keys = []
        for (_ms, ps, _mod, _lr), k in zip(combos, combo_fp):
            key = (tuple(fp[k][0]), ps)
            if key not in flt_keys:
                flt_keys.append(key)
        flt = filters(rm, [k for k in flt_keys if len(k[0])])
        print("- Scan loops: %d first-pass and %d filter sets for %d combinations in %.3f s"
              % (len(fp_keys), len(flt), len(combos), time.time() - t0))
        for (ms, ps, mod, lr), k in zip(combos, combo_fp):
            first, first_lines = fp[k]
            cuts, flt_lines = flt[(tuple(first), ps)] if len(first) else ([], [])
            d = os.path.join(outDir, combo_name(ms, ps, mod, lr if name_louvain_rounds else None))
            common = write_setting(res, d, cuts, list(first_lines) + list(flt_lines), mod, lr, _is_runtime_line,
                                   (binGroupFile, assessmentFile, chromosomeGroupFile),
                                   avgClusterPlot_outlined if plots else None, resolution)
            rows.append(dict({"minSize": ms, "psig": ps, "modularity": mod, "louvainRounds": lr,
                              "first_pass_cuts": len(first), "filtered_cuts": len(cuts)}, **common))
    write_summary(outDir, SUMMARY_COLUMNS, rows)
    print("Total run-time of the Part 1 sweep = " + str(time.time() - t_all))
    return rows


def read_summary(path):
    """sweep_summary.tsv back as rows of strings (cut_indices as a list of ints)."""
    with open(path) as fh:
        head = fh.readline().rstrip("\n").split("\t")
        out = []
        for line in fh:
            r = dict(zip(head, line.rstrip("\n").split("\t")))
            r["cut_indices"] = [int(v) for v in r["cut_indices"].split(",") if v]
            out.append(r)
    return out


def _parse_args(argv):
    p = argparse.ArgumentParser(description="Part 1 parameter sweep on one map and one GPU: the map is loaded, clustered "
                                            "and ranked once; every minSize x psig x modularity combination is evaluated "
                                            "on the resident rank matrix.")
    p.add_argument("-config", required=True, type=str, help="run_hicAssembler.py config file (hyperGeom = True)")
    p.add_argument("-minSize", type=str, help="comma-separated values (default: the config's)")
    p.add_argument("-psig", type=str, help="comma-separated values (default: the config's)")
    p.add_argument("-modularity", type=str, help="comma-separated values (default: the config's)")
    p.add_argument("-louvainRounds", type=str, help="comma-separated values (default: the config's; given: in the names)")
    p.add_argument("-device", type=int, default=0, help="GPU index (default 0)")
    p.add_argument("-out", type=str, default=None, help="output directory (default: saveFilesDirectory/sweep)")
    p.add_argument("-plots", action="store_true", help="draw the outlined clustered map of every combination")
    return p.parse_args(argv)


def grid_from_args(args, v):
    """The four value lists of the command line, each defaulting to the config's single value."""
    return tuple(parse_values(getattr(args, key), key, v[key]) if getattr(args, key) is not None else [v[key]]
                 for key in ("minSize", "psig", "modularity", "louvainRounds"))


def check_config(v):
    """None when the config can be swept, else the reason."""
    if v["hmm"] is True:
        return "the sweep evaluates the hyperGeom = True boundary finder only: hmm = True is not supported"
    if v["hyperGeom"] is not True:
        return "the sweep needs hyperGeom = True in the config"
    return None


def main(argv=None):
    args = _parse_args(argv)
    v = readConfigFileToVariables(args.config)
    reason = check_config(v)
    if reason:
        print("- ERROR - " + reason + ". Exiting...")
        sys.exit(2)
    if ensureAllVariablesAreSet(v):
        sys.exit(2)
    minSizes, psigs, modularities, louvainRounds = grid_from_args(args, v)
    out = args.out or os.path.join(v["saveFilesDirectory"], "sweep")
    runSweep(v["hicProBedFile"], v["hicProBiasFile"], v["hicProMatrixFile"], v["hicProScaffSizeFile"],
             v["dendrogramOrderFile"], v["binGroupFile"], v["assessmentFile"], v["chromosomeGroupFile"],
             minSizes, psigs, modularities, louvainRounds, out, name_louvain_rounds=args.louvainRounds is not None,
             avgClusterPlot_outlined=v["avgClusterPlot_outlined"], resolution=v["resolution"], plots=args.plots,
             device=args.device)


if __name__ == "__main__":
    main()
