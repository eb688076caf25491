"""Part 1 HMM parameter sweep: one map, one GPU, many ``minSize x modularity x convergenceRounds x lookAhead
(x louvainRounds)`` settings of the hmm = True boundary finder (HICMI_HMM=1).

    python -m hic_genome_assembler_amd.sweepHMM -config cfg.txt -minSize 5,10,15 -modularity .05,.1 \\
           -convergenceRounds 5,8 -lookAhead .2,.5 [-louvainRounds 20] [-device 0] [-out DIR] [-plots]

The map is loaded, clustered (UPGMA) and reordered once.  Every setting then runs identifyChromosomeGroupsHMM's control
flow as a generator (scaffoldToChromosomes.hmm_groups_steps) that asks for fits instead of making them.  The generators
run in lock step: each round collects the live settings' fit requests, drops duplicates (a fit is a pure function of
(c, width, fit_index) for one HICMI_HMM_SEED), and makes the remaining fits together - the X of every distinct c
resident in its own slot, the k-means++ distances of all restarts in two calls (hicmi_hmm_dist2_multi) and all Lloyd runs in one
(hicmi_hmm_kmeans_multi); EM and Viterbi stay one fit at a time.  Each setting's directory
``DIR/minSize<a>_convergenceRounds<b>_lookAhead<c>_modularity<d>[_louvainRounds<e>]/`` holds the binGroupFile,
assessmentFile and chromosomeGroupFile (config base names) that ``run_hicAssembler.py -part1`` writes with that setting,
and ``part1.log`` with the lines such a run prints from the HMM, Louvain and assessment stages (run-time lines left
out).  ``DIR/sweep_summary.tsv`` has one row per setting.  DESIGN.md section 9c.
"""
from __future__ import annotations

import argparse
import collections
import os
import sys
import time

import numpy as np

from . import scaffoldToChromosomes as s2c
from .run_hicAssembler import ensureAllVariablesAreSet, readConfigFileToVariables
from .scaffoldToChromosomes import drive, hmm_groups_steps  # noqa: F401  (drive: re-exported with the generator)
from .sweepPart1 import _fmt, _is_runtime_line, parse_values, resident_map, write_setting, write_summary

SUMMARY_COLUMNS = ["minSize", "convergenceRounds", "lookAhead", "modularity", "louvainRounds", "hmm_cuts", "groups",
                   "louvain_groups", "scaffolds_assigned", "split_scaffolds", "fits_requested", "fits_run", "cut_indices"]
# the X of all slots resident at once stays under this many bytes (HICMI_HMM_SWEEP_BYTES); more distinct c in one
# round are built in turn
SLOT_BYTES = int(os.environ.get("HICMI_HMM_SWEEP_BYTES", str(8 << 30)))


# ------------------------------------------------------------------------------------------------
def setting_name(minSize, convergenceRounds, lookAhead, modularity, louvainRounds=None):
    """minSize<a>_convergenceRounds<b>_lookAhead<c>_modularity<d>[_louvainRounds<e>]."""
    la = "False" if lookAhead is False else _fmt(lookAhead)
    name = "minSize%d_convergenceRounds%d_lookAhead%s_modularity%s" % (int(minSize), int(convergenceRounds), la,
                                                                        _fmt(modularity))
    return name if louvainRounds is None else name + "_louvainRounds%d" % int(louvainRounds)


def settings(minSizes, convergenceRounds, lookAheads, modularities, louvainRounds):
    """The grid in the order the sweep reports it."""
    return [(a, b, c, d, e) for a in minSizes for b in convergenceRounds for c in lookAheads for d in modularities
            for e in louvainRounds]


def plan_round(requests):
    """One lock-step round: ``requests`` = {setting: (c, width, fit_index)} of the live settings.  Returns the distinct
    fit keys in first-request order and {c: widest width requested at c} (the slot each c needs)."""
    keys, widest = [], {}
    for key in requests.values():
        if key not in keys:
            keys.append(key)
        widest[key[0]] = max(widest.get(key[0], 0), key[1])
    return keys, widest


def _slot_batches(n, widest, budget):
    """The distinct c of a round in groups whose X fit in ``budget`` bytes and in the context's slots."""
    from ._lib import Context
    batches, cur, used = [], [], 0
    for c in sorted(widest):
        b = (n - c) * widest[c] * 8
        if cur and (used + b > budget or len(cur) == Context.HMM_MAX_SLOTS):
            batches.append(cur)
            cur, used = [], 0
        cur.append(c)
        used += b
    if cur:
        batches.append(cur)
    return batches


class HmmBatchFitter:
    """Makes the fits of one round: HmmDevice.states for many (c, width, fit_index) keys, with the k-means restarts of
    all of them batched on the device.  Each key's states equal HmmDevice's for that key, bit for bit."""

    def __init__(self, matrix, seed=None):
        self.matrix = matrix
        self.seed = int(os.environ.get("HICMI_HMM_SEED", "0")) if seed is None else int(seed)
        self.stats = collections.Counter()

    def _tick(self, key, t0):
        self.stats[key + "_ms"] += (time.perf_counter() - t0) * 1e3

    def fit(self, keys, widest):
        ctx, n = self.matrix.ctx, self.matrix.n
        order = self.matrix.order if self.matrix.order is not None else list(range(n))
        out = {}
        for batch in _slot_batches(n, widest, SLOT_BYTES):
            t0 = time.perf_counter()
            slot = {}
            for s, c in enumerate(batch):
                ctx.hmm_load_obs_slot(s, order, c, c + widest[c])
                slot[c] = s
                self.stats["builds"] += 1
            self._tick("obs", t0)
            mine = [k for k in keys if k[0] in slot]
            out.update(self._fit_batch(ctx, n, slot, mine))
        return out

    def _fit_batch(self, ctx, n, slot, keys):
        R = s2c.HMM_KMEANS_RESTARTS
        t0 = time.perf_counter()
        # per fit: column statistics (the covariances and sklearn's tol), and every restart's random numbers - they
        # do not depend on device results, so they are drawn first
        fits = []
        for c, width, fit_index in keys:
            ctx.hmm_use_obs(slot[c])
            ctx.hmm_set_width(width)
            T = n - c
            mean, m2 = ctx.hmm_col_stats()
            var1 = m2 / (T - 1)
            tol = s2c.HMM_KMEANS_TOL * float(np.mean(m2 / T))
            draws = []
            for restart in range(R):
                rng = np.random.default_rng([self.seed, fit_index, restart])
                first = int(rng.integers(T))
                draws.append((first, rng.uniform(size=2)))
            fits.append((slot[c], width, T, tol, var1, draws))
        # kmeans_plusplus_rows for all restarts: the first rows' distances, the candidates, their distances
        probs = [(s, w, [first]) for s, w, _T, _tol, _v, draws in fits for first, _u in draws]
        closest = ctx.hmm_dist2_multi(probs)
        cands = []
        for (s, w, T, _tol, _v, draws), j0 in zip(fits, range(0, len(probs), R)):
            for r, (_first, u) in enumerate(draws):
                cl = closest[j0 + r][0]
                rand_vals = u * cl.sum()
                cands.append((s, w, np.minimum(np.searchsorted(np.cumsum(cl), rand_vals), T - 1)))
        cdist = ctx.hmm_dist2_multi(cands)
        km = []
        for j, (s, w, cand) in enumerate(cands):
            dist = np.minimum(closest[j][0], cdist[j])
            best = int(np.argmin(dist.sum(axis=1)))
            f = fits[j // R]
            km.append((s, w, (probs[j][2][0], int(cand[best])), s2c.HMM_KMEANS_MAX_ITER, f[3]))
        self._tick("seed", t0)
        t0 = time.perf_counter()
        res = ctx.hmm_kmeans_multi(km)
        self._tick("kmeans", t0)
        self.stats["kmeans_iterations"] += sum(r[2] for r in res)
        self.stats["kmeans_runs"] += len(res)
        out = {}
        for i, key in enumerate(keys):
            best = None
            for centers, inertia, _it in res[i * R:(i + 1) * R]:
                if best is None or inertia < best[1]:
                    best = (centers, inertia)
            s, width, _T, _tol, var1, _d = fits[i]
            covars = np.vstack([var1 + s2c.HMM_MIN_COVAR, var1 + s2c.HMM_MIN_COVAR])
            t0 = time.perf_counter()
            ctx.hmm_use_obs(s)
            ctx.hmm_set_width(width)
            means, covars, transmat, hist = ctx.hmm_fit(s2c.HMM_STARTPROB, best[0], covars, s2c.HMM_TRANSMAT,
                                                        s2c.HMM_N_ITER, s2c.HMM_TOL)
            self._tick("fit", t0)
            t0 = time.perf_counter()
            out[key] = ctx.hmm_decode(s2c.HMM_STARTPROB, means, covars, transmat)
            self._tick("decode", t0)
            self.stats["fits"] += 1
            self.stats["em_iterations"] += len(hist)
        return out

    def report(self):
        s = self.stats
        sys.stderr.write("[hicmi] hmm sweep: %d fits, %d EM iterations, %d k-means runs, %d k-means iterations, %d X "
                         "builds; ms: obs %.1f, k-means++ seeding %.1f, k-means %.1f, fit %.1f, decode %.1f\n"
                         % (s["fits"], s["em_iterations"], s["kmeans_runs"], s["kmeans_iterations"], s["builds"],
                            s["obs_ms"], s["seed_ms"], s["kmeans_ms"], s["fit_ms"], s["decode_ms"]))


def run_lock_step(n, grid, fitter):
    """The HMM boundaries of every setting of ``grid`` [(minSize, convergenceRounds, lookAhead, modularity,
    louvainRounds)]: (cut indices, printed lines, fits requested, fits run) per setting.  ``fitter.fit(keys, widest)``
    returns {key: states}."""
    logs = [[] for _ in grid]
    gens, reqs, result = [], {}, {}
    requested, run = [0] * len(grid), [0] * len(grid)
    for i, (ms, cr, la, mod, lr) in enumerate(grid):
        g = hmm_groups_steps(n, minSize=ms, modularity=mod, convergenceRounds=cr, lookAhead=la, louvainRounds=lr,
                             emit=logs[i].append)
        gens.append(g)
        try:
            reqs[i] = next(g)
        except StopIteration as stop:
            result[i] = stop.value
    cache = {}
    while reqs:
        keys, widest = plan_round(reqs)
        todo = [k for k in keys if k not in cache]
        if todo:
            cache.update(fitter.fit(todo, {c: w for c, w in widest.items() if any(k[0] == c for k in todo)}))
        for i in sorted(reqs):
            key = reqs[i]
            requested[i] += 1
            if key in todo:
                todo.remove(key)                             # the first setting to ask for a fit is charged with it
                run[i] += 1
            try:
                reqs[i] = gens[i].send(cache[key])
            except StopIteration as stop:
                result[i] = stop.value
                del reqs[i]
    return [(result[i], logs[i], requested[i], run[i]) for i in range(len(grid))]


def _is_hmm_runtime_line(line):
    return (_is_runtime_line(line) or line.startswith("HMM rounds completed in")
            or line.startswith("Total time to identify chromosome boundries"))


def runSweep(hicProBedFile, hicProBiasFile, hicProMatrixFile, hicProScaffSizeFile, dendrogramOrderFile,
             binGroupFile, assessmentFile, chromosomeGroupFile, minSizes, modularities, convergenceRounds, lookAheads,
             louvainRounds, outDir, name_louvain_rounds=None, avgClusterPlot_outlined=None, resolution=100000,
             plots=False, device=0):
    """S2C:1117-1167 with hmm = True for every setting of the grid on one resident map (see the module docstring).
    Returns the summary rows (dicts keyed by SUMMARY_COLUMNS, cut_indices a list)."""
    if not s2c.hmm_enabled():
        raise NotImplementedError("the HMM sweep needs HICMI_HMM=1 (the hmm = True boundary finder is opt-in)")
    if name_louvain_rounds is None:
        name_louvain_rounds = len(louvainRounds) > 1
    grid = settings(minSizes, convergenceRounds, lookAheads, modularities, louvainRounds)
    os.makedirs(outDir, exist_ok=True)
    print("### Part 1 HMM sweep: %d settings ###" % len(grid))
    t_all = time.time()
    rows = []
    with resident_map(hicProBedFile, hicProBiasFile, hicProMatrixFile, hicProScaffSizeFile, dendrogramOrderFile,
                      device) as res:
        n = res.adjMat.n
        t0 = time.time()
        fitter = HmmBatchFitter(res.adjMat)
        found = run_lock_step(n, grid, fitter)
        print("- HMM fits: %d requested, %d run for %d settings in %.3f s"
              % (sum(f[2] for f in found), sum(f[3] for f in found), len(grid), time.time() - t0))
        if os.environ.get("HICMI_HMM_PROFILE") == "1":
            fitter.report()
        for (ms, cr, la, mod, lr), (cuts, lines, n_req, n_run) in zip(grid, found):
            log = [ln for ln in "\n".join(lines).split("\n") if not _is_hmm_runtime_line(ln)]
            d = os.path.join(outDir, setting_name(ms, cr, la, mod, lr if name_louvain_rounds else None))
            common = write_setting(res, d, cuts, log, mod, lr, _is_hmm_runtime_line,
                                   (binGroupFile, assessmentFile, chromosomeGroupFile),
                                   avgClusterPlot_outlined if plots else None, resolution)
            rows.append(dict({"minSize": ms, "convergenceRounds": cr, "lookAhead": la, "modularity": mod,
                              "louvainRounds": lr, "hmm_cuts": len(cuts), "fits_requested": n_req, "fits_run": n_run},
                             **common))
    write_summary(outDir, SUMMARY_COLUMNS, rows)
    print("Total run-time of the Part 1 HMM sweep = " + str(time.time() - t_all))
    return rows


def _parse_args(argv):
    p = argparse.ArgumentParser(description="Part 1 HMM parameter sweep on one map and one GPU (hmm = True, "
                                            "HICMI_HMM=1): the map is loaded and clustered once; the HMM fits of every "
                                            "setting are made in lock step, shared fits once.")
    p.add_argument("-config", required=True, type=str, help="run_hicAssembler.py config file (hmm = True)")
    for key in ("minSize", "modularity", "convergenceRounds", "lookAhead"):
        p.add_argument("-" + key, type=str, help="comma-separated values (default: the config's)")
    p.add_argument("-louvainRounds", type=str, help="comma-separated values (default: the config's; given: in the names)")
    p.add_argument("-device", type=int, default=0, help="GPU index (default 0)")
    p.add_argument("-out", type=str, default=None, help="output directory (default: saveFilesDirectory/sweep_hmm)")
    p.add_argument("-plots", action="store_true", help="draw the outlined clustered map of every setting")
    return p.parse_args(argv)


def grid_from_args(args, v):
    """The five value lists of the command line, each defaulting to the config's single value."""
    return tuple(parse_values(getattr(args, key), key, v[key]) if getattr(args, key) is not None else [v[key]]
                 for key in ("minSize", "modularity", "convergenceRounds", "lookAhead", "louvainRounds"))


def check_config(v):
    """None when the config can be swept, else the reason."""
    if v["hmm"] is not True or v["hyperGeom"] is True:
        return "the HMM sweep needs hmm = True and hyperGeom = False in the config"
    if not s2c.hmm_enabled():
        return "the HMM sweep needs HICMI_HMM=1 (the hmm = True boundary finder is opt-in)"
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
    minSizes, modularities, convergenceRounds, lookAheads, louvainRounds = grid_from_args(args, v)
    out = args.out or os.path.join(v["saveFilesDirectory"], "sweep_hmm")
    runSweep(v["hicProBedFile"], v["hicProBiasFile"], v["hicProMatrixFile"], v["hicProScaffSizeFile"],
             v["dendrogramOrderFile"], v["binGroupFile"], v["assessmentFile"], v["chromosomeGroupFile"],
             minSizes, modularities, convergenceRounds, lookAheads, louvainRounds, out,
             name_louvain_rounds=args.louvainRounds is not None, avgClusterPlot_outlined=v["avgClusterPlot_outlined"],
             resolution=v["resolution"], plots=args.plots, device=args.device)


if __name__ == "__main__":
    main()
