#!/usr/bin/env python3
"""Raw maps from read pairs on the device (hicmi_map_*, hicmi_build_maps): the combining kernel against one
atomic add per pair, and the one-pass driver on a text file.

    python profiles/buildmap_bench.py [--bins 16000] [--pairs 8000000] [--lines 3000000] [--repeats 3] [--no-text] [--out FILE]

The pairs are drawn from the 16,000-bin raw map of profiles/ice_bench.py (make_raw_counts, seed 1): the map is thinned
cell by cell (binomial) to about --pairs read pairs, every pair gets positions inside its two bins and the list is sorted
as HiC-Pro sorts its merged file (scaffold 1, position 1, ...).
  accumulate  Context.map_add_pairs on the host arrays, no text: HICMI_BUILDMAP_PLAIN=1 and =0 alternated, --repeats timed
              calls each after one warm-up call each, host clock around the call (checking the pairs on the host, staging
              and upload, the kernel, one synchronise).  The kernel times proper come from a `rocprofv3 --kernel-trace
              --stats` run of this script with --no-text.
  text        --lines of such pairs written as a twelve-column allValidPairs file; hicmi_parse_valid_pairs alone over the
              file (the parse-bound time), then hicmi_build_maps at one resolution and at four, with the default chunk and
              with chunks of 2^19 pairs.
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
FORMS = (("combine", "0"), ("plain", "1"))


def thinned(counts, want, seed):
    """The upper triangle of ``counts`` with every read pair kept with probability want / total, mirrored."""
    rng = np.random.default_rng(seed)
    upper = np.triu(counts)
    total = upper.sum()
    keep = rng.binomial(upper.astype(np.int64), min(1.0, want / total)).astype(np.float64)
    return keep + np.triu(keep, 1).T, float(total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--lines", type=int, default=3000000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--no-text", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, synth

    n = args.bins
    t0 = time.time()
    lay = synth.make_layout(n, seed=1)
    counts, lay = synth.make_raw_counts(lay, seed=1)
    sample, total = thinned(counts, args.pairs, seed=2)
    text_sample = None if args.no_text else thinned(counts, args.lines, seed=3)[0]
    del counts
    pairs = synth.draw_valid_pairs(lay, sample, seed=1, sort=True)
    sizes, r = lay.scaffold_sizes_bp, lay.resolution
    out = {"bins": n, "read_pairs_of_the_map": total, "pairs": int(len(pairs[0])), "make_s": round(time.time() - t0, 1),
           "repeats": args.repeats}

    # ---- accumulate: map_add_pairs on host arrays
    def count(flag, want=False):
        os.environ["HICMI_BUILDMAP_PLAIN"] = flag
        with _lib.Context(0) as ctx:
            ctx.map_begin(sizes, r)
            ctx.synchronize()
            t = time.perf_counter()
            ctx.map_add_pairs(*pairs)
            dt = time.perf_counter() - t
            if not want:
                return dt, None
            ctx.map_finish()
            return dt, ctx.contacts_host()
    maps = {name: count(flag, want=True)[1] for name, flag in FORMS}          # warm-up, and the results
    times = {name: [] for name, _f in FORMS}
    for _k in range(args.repeats):
        for name, flag in FORMS:
            times[name].append(count(flag)[0])
    upper = np.triu(maps["plain"])
    out["accumulate"] = {
        "same_bytes": bool(maps["plain"].tobytes() == maps["combine"].tobytes() == sample.tobytes()),
        "distinct_cells": int(np.count_nonzero(upper)), "largest_cell": float(upper.max()),
        "call_ms": {name: [round(v * 1e3, 3) for v in times[name]] for name in times},
        "combine_slowest_beats_plain_fastest": bool(max(times["combine"]) < min(times["plain"]))}
    del maps, upper, sample
    os.environ.pop("HICMI_BUILDMAP_PLAIN", None)

    # ---- text: the parser alone, then the driver
    if not args.no_text:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "bench.allValidPairs")
            t0 = time.time()
            n_lines = synth.write_valid_pairs(path, lay, text_sample, seed=4, sort=True)
            rec = {"lines": n_lines, "file_MB": round(os.path.getsize(path) / 1e6, 1), "write_s": round(time.time() - t0, 1)}
            names = lay.scaffold_names
            parse = []
            for _k in range(args.repeats + 1):
                t = time.perf_counter()
                got = _lib.parse_valid_pairs(path, names, sizes, threads=args.threads)
                parse.append(round(time.perf_counter() - t, 4))
                assert got[5] == (n_lines, n_lines, 0, 0)
            rec["parse_only_s"] = parse

            def drive(resolutions, chunk):
                os.environ.pop("HICMI_BUILDMAP_CHUNK_PAIRS", None)
                if chunk:
                    os.environ["HICMI_BUILDMAP_CHUNK_PAIRS"] = str(chunk)
                ctxs = [_lib.Context(0) for _r in resolutions]
                try:
                    t = time.perf_counter()
                    stats = _lib.build_maps(path, names, sizes, resolutions, ctxs, threads=args.threads)
                    dt = time.perf_counter() - t
                    assert stats[:4] == (n_lines, n_lines, 0, 0)
                    return round(dt, 4), stats[4], ctxs[0].contacts_host() if len(resolutions) == 1 else None
                finally:
                    for c in ctxs:
                        c.close()
            four = [r, r * 3 // 2, 2 * r, r * 5 // 2]
            _dt, _chunks, built = drive([r], None)                            # warm-up, and the result
            rec["equals_the_sampled_map"] = bool(built.tobytes() == text_sample.tobytes())
            del built
            for chunk in (None, 1 << 19):
                key = "default_chunk" if chunk is None else "chunk_%d" % chunk
                rec[key] = {"one_resolution_s": [], "four_resolutions_s": [], "each_of_the_four_alone_s": []}
                for _k in range(args.repeats):
                    dt, chunks, _m = drive([r], chunk)
                    rec[key]["one_resolution_s"].append(dt)
                    rec[key]["chunks"] = chunks
                    rec[key]["four_resolutions_s"].append(drive(four, chunk)[0])
                rec[key]["each_of_the_four_alone_s"] = [drive([q], chunk)[0] for q in four]
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
