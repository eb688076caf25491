#!/usr/bin/env python3
"""Rebinning on the device (hicmi_rebin): the default kernels against HICMI_REBIN_PLAIN=1 on the
16,000-bin raw map of profiles/ice_bench.py.

    python profiles/rebin_bench.py [--bins 16000] [--factors 2,5] [--repeats 3] [--out FILE]

The fine map is uploaded once; per timed call a second context adopts it (no copy) and the wall time of its
``hicmi_rebin`` is taken (host clock around the call, which synchronises the stream after the rebinning kernels).  A call
is more than its kernels - it allocates the m x m result and the row-sum vectors and uploads group_start - so the kernel
times proper come from a `rocprofv3 --kernel-trace` run of this script (k_rebin, k_rebin_mirror, k_rebin_plain, by name).
The two forms are alternated, after one warm-up call each.  Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_MEASURED_TBS = 6.29          # float4 copy on MI355X
ICE_ROWDOT_TBS = 4.87            # k_ice_rowdot on the same map
FORMS = (("default", {}), ("plain", {"HICMI_REBIN_PLAIN": "1"}))


def bytes_moved(form, n, m):
    """Algorithmic bytes.  default: the upper block triangle of the fine map read, the upper triangle of the result
    written, read again by the mirror pass and written as the lower triangle.  plain: every cell reads its block - the
    upper block triangle twice - and writes itself."""
    if form == "plain":
        return 8.0 * (n * n + m * m)
    return 4.0 * n * n + 12.0 * m * m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--factors", default="2,5")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, hostio, synth

    n = args.bins
    t0 = time.time()
    lay = synth.make_layout(n, seed=1)
    counts, lay = synth.make_raw_counts(lay, seed=1, dead_bins=(n // 3,))
    bins = [hostio.Bin(int(i), lay.scaffold_names[s], int(a), int(b), 1., 0.)
            for i, s, a, b in zip(lay.bin_ids, lay.scaffold_of_bin, lay.start, lay.stop)]
    build_s = time.time() - t0
    fine = _lib.Context(0)
    fine.set_contacts(counts)
    pairs = float(np.triu(counts).sum())
    del counts
    ptr, _n, ld = fine.contacts_device()

    def call(env, group_start, want=False):
        os.environ.pop("HICMI_REBIN_PLAIN", None)
        os.environ.update(env)
        with _lib.Context(0) as ctx:
            ctx.set_contacts_device(ptr, n, ld, keepalive=fine)
            ctx.synchronize()
            t = time.perf_counter()
            ctx.rebin(group_start)
            dt = time.perf_counter() - t
            return dt, (ctx.contacts_host() if want else None)

    out = {"bins": n, "build_s": round(build_s, 1), "repeats": args.repeats, "read_pairs": pairs, "factors": {}}
    for k in [int(v) for v in args.factors.split(",")]:
        _coarse, g = hostio.rebin_bins(bins, k)
        m = len(g) - 1
        maps = {}
        for name, env in FORMS:                            # warm-up: code objects, pinned staging; and the results
            maps[name] = call(env, g, want=True)[1]
        times = {name: [] for name, _env in FORMS}
        for _r in range(args.repeats):
            for name, env in FORMS:
                times[name].append(call(env, g)[0])
        rec = {"coarse_bins": m, "read_pairs_kept": bool(np.triu(maps["default"]).sum() == pairs),
               "same_bytes_as_default": {name: bool(maps[name].tobytes() == maps["default"].tobytes()) for name, _e in FORMS},
               "symmetric": bool(np.array_equal(maps["default"], maps["default"].T)), "forms": {}}
        for name in list(times):
            ms = np.array(times[name]) * 1e3
            f = {"call_ms": [round(v, 3) for v in ms], "call_ms_median": round(float(np.median(ms)), 3),
                 "bytes": bytes_moved(name, n, m)}
            f["TB_per_s_of_the_call"] = round(f["bytes"] / (f["call_ms_median"] * 1e-3) / 1e12, 3)
            rec["forms"][name] = f
        d, p = rec["forms"]["default"], rec["forms"]["plain"]
        rec["plain_over_default"] = round(p["call_ms_median"] / d["call_ms_median"], 3)
        rec["default_share_of_measured_hbm"] = round(d["TB_per_s_of_the_call"] / HBM_MEASURED_TBS, 3)
        rec["default_over_ice_rowdot"] = round(d["TB_per_s_of_the_call"] / ICE_ROWDOT_TBS, 3)
        out["factors"][str(k)] = rec
    fine.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
