#!/usr/bin/env python3
"""ICE balancing on the device (hicmi_ice_balance): the read-only default path against
HICMI_ICE_INPLACE=1 on a 16,000-bin raw map in the shape of bench.py's map.

    python profiles/ice_bench.py [--bins 16000] [--repeats 3] [--out FILE]

Per path, alternated, after one warm-up call each: the wall time (host clock around the call, which ends in a stream
synchronise) of a call with a FIXED iteration count - eps = 0 never stops - at `--iters-long` and at `--iters-short`
iterations; their difference over the difference in iterations is the time per iteration, free of the call's fixed cost
(mask, the raw map's row sums, the final k_ice_apply pass, downloads).  Then one call each with HiC-Pro's settings
(eps 0.1, 100 iterations at most): iterations, time, and the largest relative difference between the two paths' maps
and biases.  The raw map is uploaded again before every call (a call rewrites the resident matrix); uploads are not timed.
Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_MEASURED_TBS = 6.29          # float4 copy on MI355X; the spec figure is 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters-long", type=int, default=25)
    ap.add_argument("--iters-short", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, iceNormalize, synth

    n = args.bins
    t0 = time.time()
    lay = synth.make_layout(n, seed=1)
    counts, lay = synth.make_raw_counts(lay, seed=1, dead_bins=(n // 3,))
    build_s = time.time() - t0
    ctx = _lib.Context(0)

    def call(inplace, max_iter, eps, want_map=False):
        if inplace:
            os.environ["HICMI_ICE_INPLACE"] = "1"
        else:
            os.environ.pop("HICMI_ICE_INPLACE", None)
        ctx.set_contacts(counts)
        weights, _seq = ctx.row_sums()
        mask = iceNormalize.build_mask(weights, None, 0.02)[0]
        ctx.synchronize()
        t = time.perf_counter()
        bias, iters, delta = ctx.ice_balance(mask, max_iter, eps)
        dt = time.perf_counter() - t
        return dt, iters, delta, bias, (ctx.contacts_host() if want_map else None), int(mask.sum())

    paths = (("default", False), ("inplace", True))
    for _name, ip in paths:                                # warm-up: code objects, buffers, pinned staging
        call(ip, 2, 0.0)
    times = {name: {"long": [], "short": []} for name, _ip in paths}
    for _r in range(args.repeats):
        for which, iters in (("long", args.iters_long), ("short", args.iters_short)):
            for name, ip in paths:
                dt, done, _d, _b, _m, _k = call(ip, iters, 0.0)
                assert done == iters
                times[name][which].append(dt)
    out = {"bins": n, "build_s": round(build_s, 1), "repeats": args.repeats, "iters_long": args.iters_long,
           "iters_short": args.iters_short, "paths": {}}
    for name, _ip in paths:
        lo, sh = np.array(times[name]["long"]), np.array(times[name]["short"])
        per_it = (lo - sh) / (args.iters_long - args.iters_short)
        out["paths"][name] = {
            "call_ms_long": [round(v * 1e3, 3) for v in lo], "call_ms_short": [round(v * 1e3, 3) for v in sh],
            "ms_per_iteration": [round(v * 1e3, 4) for v in per_it],
            "ms_per_iteration_median": round(float(np.median(per_it)) * 1e3, 4)}
    d = out["paths"]["default"]
    d["bytes_per_iteration"] = 8.0 * n * n
    d["TB_per_s"] = round(8.0 * n * n / (d["ms_per_iteration_median"] * 1e-3) / 1e12, 3)
    d["share_of_measured_hbm"] = round(d["TB_per_s"] / HBM_MEASURED_TBS, 3)
    res = {}
    for name, ip in paths:
        dt, iters, delta, bias, X, masked = call(ip, 100, 0.1, want_map=True)
        res[name] = (bias, X)
        out["paths"][name]["hicpro_settings"] = {"call_ms": round(dt * 1e3, 3), "iterations": iters, "delta": delta,
                                                 "masked": masked}
    (b0, X0), (b1, X1) = res["default"], res["inplace"]
    nz = X1 != 0
    ok = ~np.isnan(b1)
    out["default_vs_inplace"] = {
        "values_max_rel": float((np.abs(X0 - X1)[nz] / np.abs(X1[nz])).max()),
        "biases_max_rel": float((np.abs(b0[ok] - b1[ok]) / np.abs(b1[ok])).max()),
        "same_zero_pattern": bool(np.array_equal(X0 == 0, ~nz)), "symmetric": bool(np.array_equal(X0, X0.T)),
        "same_nan": bool(np.array_equal(np.isnan(b0), np.isnan(b1)))}
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
