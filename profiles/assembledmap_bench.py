#!/usr/bin/env python3
"""Maps of the assembled genome on the device (hicmi_map_begin_lifted, hicmi_pair_stats, hicmi_lift_maps):
the combining kernel against one atomic add per pair on a lifted build, the statistics kernel, and the one-pass driver on
a text file.

    python profiles/assembledmap_bench.py [--bins 16000] [--pairs 8000000] [--inter 0.02,0.0002] [--lines 3000000]
                                          [--repeats 3] [--no-text] [--out FILE]

Per value of --inter the pairs are drawn as profiles/buildmap_bench.py draws them - the 16,000-bin make_raw_counts map
(seed 1) thinned cell by cell to about --pairs read pairs, positions inside the bins, sorted as HiC-Pro sorts - and lifted by
the map's true layout: the scaffolds of a planted chromosome by rank, reversed where planted so, 100 bp between them.  At
inter = 0.02 (the bench map) about 5 % of the pairs are cis; the second value makes most of them cis, as in a real
library, and is the case that decides the default of HICMI_LIFTMAP_PLAIN.
  accumulate  Context.map_add_pairs on a lifted build, HICMI_LIFTMAP_PLAIN=1 and =0 alternated, --repeats timed calls each
              after one warm-up call each, host clock around the call; Context.pair_stats the same number of times.  The
              kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this script with --no-text.
  text        --lines pairs of the first --inter as a twelve-column allValidPairs file: hicmi_lift_maps at one resolution
              and at four in one call, against the four one call each.
Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
FORMS = (("combine", "0"), ("plain", "1"))
GAP = 100


def true_layout(lay):
    """(lift_seq, lift_off, lift_rev, seq_sizes) of the planted chromosomes."""
    S = len(lay.scaffold_names)
    seq, off, rev = np.zeros(S, np.int32), np.zeros(S, np.int64), np.zeros(S, np.uint8)
    seq_sizes = []
    for c in range(int(lay.scaffold_chrom.max()) + 1):
        at = 0
        for k, s in enumerate(sorted(np.flatnonzero(lay.scaffold_chrom == c).tolist(), key=lambda s: lay.scaffold_rank[s])):
            at += GAP if k else 0
            seq[s], off[s], rev[s] = c, at, lay.scaffold_orient[s] < 0
            at += int(lay.scaffold_sizes_bp[s])
        seq_sizes.append(at)
    return seq, off, rev, np.asarray(seq_sizes, np.int64)


def main():
    from buildmap_bench import thinned
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--inter", default="0.02,0.0002")
    ap.add_argument("--lines", type=int, default=3000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--no-text", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, synth

    n = args.bins
    lay0 = synth.make_layout(n, seed=1)
    out = {"bins": n, "repeats": args.repeats, "gap": GAP, "cases": []}
    text_case = None
    for inter in [float(x) for x in args.inter.split(",")]:
        t0 = time.time()
        counts, lay = synth.make_raw_counts(lay0, seed=1, inter=inter)
        sample, total = thinned(counts, args.pairs, seed=2)
        if text_case is None and not args.no_text:
            text_case = (lay, thinned(counts, args.lines, seed=3)[0])
        del counts
        pairs = synth.draw_valid_pairs(lay, sample, seed=1, sort=True)
        del sample
        sizes, r = lay.scaffold_sizes_bp, lay.resolution
        tables = true_layout(lay)
        rec = {"inter": inter, "read_pairs_of_the_map": total, "pairs": int(len(pairs[0])), "sequences": int(len(tables[3])),
               "make_s": round(time.time() - t0, 1)}

        def count(flag, want=False):
            os.environ["HICMI_LIFTMAP_PLAIN"] = flag
            with _lib.Context(0) as ctx:
                ctx.map_begin_lifted(sizes, *tables, r)
                ctx.synchronize()
                t = time.perf_counter()
                ctx.map_add_pairs(*pairs)
                dt = time.perf_counter() - t
                if not want:
                    return dt, None
                ctx.map_finish()
                return dt, ctx.contacts_host()
        maps = {name: count(flag, want=True)[1] for name, flag in FORMS}      # warm-up, and the results
        times = {name: [] for name, _f in FORMS}
        for _k in range(args.repeats):
            for name, flag in FORMS:
                times[name].append(count(flag)[0])
        os.environ.pop("HICMI_LIFTMAP_PLAIN", None)
        upper = np.triu(maps["plain"])
        rec["accumulate"] = {
            "same_bytes": bool(maps["plain"].tobytes() == maps["combine"].tobytes()), "bins_of_the_lifted_map": int(len(upper)),
            "pairs_counted": float(upper.sum()), "distinct_cells": int(np.count_nonzero(upper)), "largest_cell": float(upper.max()),
            "call_ms": {name: [round(v * 1e3, 3) for v in times[name]] for name in times},
            "combine_slowest_beats_plain_fastest": bool(max(times["combine"]) < min(times["plain"]))}
        del maps, upper
        stat_ms = []
        with _lib.Context(0) as ctx:
            for _k in range(args.repeats + 1):
                t = time.perf_counter()
                decay, cis, trans, unlifted = ctx.pair_stats(*pairs, sizes, *tables)
                stat_ms.append(round((time.perf_counter() - t) * 1e3, 3))
        n_cis, n_trans = int(cis.sum()), int(trans.sum()) // 2
        rec["pair_stats"] = {"call_ms": stat_ms, "cis": n_cis, "trans": n_trans, "cis_fraction": round(n_cis / (n_cis + n_trans), 4),
                             "unlifted": int(unlifted[0]), "largest_decay_slot": int(decay.max()),
                             "decay_slots_used": int(np.count_nonzero(decay)), "largest_cis_counter": int(cis.max())}
        out["cases"].append(rec)
        del pairs

    if text_case is not None:
        lay, text_sample = text_case
        sizes, r, names = lay.scaffold_sizes_bp, lay.resolution, lay.scaffold_names
        tables = true_layout(lay)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "bench.allValidPairs")
            n_lines = synth.write_valid_pairs(path, lay, text_sample, seed=4, sort=True)
            rec = {"lines": n_lines, "file_MB": round(os.path.getsize(path) / 1e6, 1)}

            def drive(resolutions, lifted=True):
                ctxs = [_lib.Context(0) for _r in resolutions]
                try:
                    t = time.perf_counter()
                    if lifted:
                        stats = _lib.lift_maps(path, names, sizes, *tables, resolutions, ctxs, threads=args.threads)[0]
                    else:
                        stats = _lib.build_maps(path, names, sizes, resolutions, ctxs, threads=args.threads)
                    dt = time.perf_counter() - t
                    assert stats[:4] == (n_lines, n_lines, 0, 0)
                    return round(dt, 4)
                finally:
                    for c in ctxs:
                        c.close()
            four = [r, r * 3 // 2, 2 * r, r * 5 // 2]
            drive([r])                                                          # warm-up
            drive([r], lifted=False)
            rec["lift_maps_one_resolution_s"] = [drive([r]) for _k in range(args.repeats)]
            rec["lift_maps_four_resolutions_s"] = [drive(four) for _k in range(args.repeats)]
            rec["lift_maps_each_of_the_four_alone_s"] = [drive([q]) for q in four]
            rec["build_maps_one_resolution_s"] = [drive([r], lifted=False) for _k in range(args.repeats)]
            rec["build_maps_four_resolutions_s"] = [drive(four, lifted=False) for _k in range(args.repeats)]
            rec["resolutions"] = four
            out["text"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
