#!/usr/bin/env python3
"""Read pairs moved to the pieces of cut scaffolds on the device (hicmi_split_pairs, hicmi_split_maps): the
combining kernel against the literal one, with about 1 % of the scaffolds cut and with none cut, and the one-pass driver on a
text file beside hicmi_build_maps on the same file.

    python profiles/split_bench.py [--bins 16000] [--pairs 8000000] [--lines 3000000] [--cut 0.01] [--repeats 3] [--no-text]
                                   [--out FILE]

The pairs are the ones profiles/buildmap_bench.py draws: the 16,000-bin make_raw_counts map thinned to about --pairs read
pairs, sorted as HiC-Pro sorts.  A cut scaffold - every 1 / --cut-th one, longest first among equals - gets two cuts, at a
third and at two thirds of its length.
  pairs   Context.split_pairs, HICMI_SPLIT_PLAIN=0 and =1 alternated, --repeats timed calls each after one warm-up call each,
          host clock around the call (upload, kernel, download of the moved chunk).
  text    --lines pairs as a twelve-column allValidPairs file: split_maps at the map's resolution in both forms, and
          build_maps on the same file, whole calls.
The kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this script with --no-text.
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


def cut_tables(names, sizes, fraction):
    """The pieces with every round(1 / fraction)-th scaffold of three bases or more cut at a third and at two thirds."""
    from hic_genome_assembler_amd import splitScaffolds
    every = int(round(1 / fraction)) if fraction > 0 else 0
    cuts = {names[s]: [int(sizes[s]) // 3, 2 * int(sizes[s]) // 3] for s in range(len(names)) if every and s % every == 0 and sizes[s] >= 3}
    return splitScaffolds.make_pieces(names, sizes, cuts)


def main():
    from buildmap_bench import thinned
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--lines", type=int, default=3000000)
    ap.add_argument("--cut", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--no-text", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, synth

    t0 = time.time()
    lay = synth.make_layout(args.bins, seed=1)
    counts, lay = synth.make_raw_counts(lay, seed=1)
    sample, total = thinned(counts, args.pairs, seed=2)
    text_sample = None if args.no_text else thinned(counts, args.lines, seed=3)[0]
    del counts
    pairs = synth.draw_valid_pairs(lay, sample, seed=1, sort=True)
    del sample
    names, sizes = lay.scaffold_names, lay.scaffold_sizes_bp
    out = {"bins": args.bins, "scaffolds": len(names), "read_pairs_of_the_map": total, "pairs": int(len(pairs[0])),
           "repeats": args.repeats, "make_s": round(time.time() - t0, 1), "cases": []}
    cases = (("cut", cut_tables(names, sizes, args.cut)), ("uncut", cut_tables(names, sizes, 0)))
    for label, pieces in cases:
        def move(flag):
            os.environ["HICMI_SPLIT_PLAIN"] = flag
            with _lib.Context(0) as ctx:
                ctx.synchronize()
                t = time.perf_counter()
                got = ctx.split_pairs(*pairs, sizes, pieces.piece_first, pieces.piece_start)
                return time.perf_counter() - t, got
        results = {name: move(flag)[1] for name, flag in FORMS}                 # warm-up, and the results
        times = {name: [] for name, _f in FORMS}
        for _k in range(args.repeats):
            for name, flag in FORMS:
                times[name].append(move(flag)[0])
        same = all(a.tobytes() == b.tobytes() for a, b in zip(results["plain"], results["combine"]))
        c = results["plain"][4]
        out["cases"].append({"case": label, "scaffolds_cut": len(pieces.applied), "pieces": len(pieces.names), "same_bytes": bool(same),
                             "within": int(c[0].sum()), "sibling_pairs": int(c[1].sum()) // 2, "other_pairs": int(c[2].sum()) // 2,
                             "counters_used": int(np.count_nonzero(c)),
                             "call_ms": {name: [round(v * 1e3, 3) for v in times[name]] for name in times}})
    os.environ.pop("HICMI_SPLIT_PLAIN", None)
    del pairs

    if text_sample is not None:
        r = lay.resolution
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "bench.allValidPairs")
            n_lines = synth.write_valid_pairs(path, lay, text_sample, seed=4, sort=True)
            rec = {"lines": n_lines, "file_MB": round(os.path.getsize(path) / 1e6, 1), "resolution": r}

            def drive(pieces, flag):
                if flag is not None:
                    os.environ["HICMI_SPLIT_PLAIN"] = flag
                with _lib.Context(0) as ctx:
                    t = time.perf_counter()
                    if pieces is None:
                        stats = _lib.build_maps(path, names, sizes, [r], [ctx], threads=args.threads)
                    else:
                        stats = _lib.split_maps(path, names, sizes, pieces.piece_first, pieces.piece_start, [r], [ctx], threads=args.threads)[0]
                    dt = time.perf_counter() - t
                assert stats[:4] == (n_lines, n_lines, 0, 0)
                return round(dt, 4)
            drive(None, None)                                                       # warm-up
            rec["build_maps_s"] = [drive(None, None) for _k in range(args.repeats)]
            for label, pieces in cases:
                for name, flag in FORMS:
                    drive(pieces, flag)
                    rec["split_maps_%s_%s_s" % (label, name)] = [drive(pieces, flag) for _k in range(args.repeats)]
            rec["build_maps_again_s"] = [drive(None, None) for _k in range(args.repeats)]
            os.environ.pop("HICMI_SPLIT_PLAIN", None)
            t = time.perf_counter()
            pieces = cases[0][1]
            _lib.split_valid_pairs(path, os.path.join(tmp, "split.allValidPairs"), names, sizes, pieces.piece_first, pieces.piece_start,
                                   pieces.names, threads=args.threads)
            rec["split_valid_pairs_s"] = round(time.perf_counter() - t, 4)
            out["text"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
