#!/usr/bin/env python3
"""End support on the device (hicmi_ends_begin / _add_pairs / _finish / _file): the combining count kernel
against one atomic add per linked pair, at a short and at the longest reach, and the one-pass driver on a text file.

    python profiles/ends_bench.py [--bins 16000] [--pairs 8000000] [--inter 0.02] [--lines 3000000] [--window 50000]
                                  [--reach 2,64] [--repeats 3] [--no-text] [--out FILE]

The pairs are the ones profiles/assembledmap_bench.py draws - the 16,000-bin make_raw_counts map thinned to about --pairs read
pairs, sorted as HiC-Pro sorts, per value of --inter - and the assembly is the map's true layout with 100 bp between
neighbours.
  count   Context.ends_add_pairs, HICMI_ENDS_PLAIN=1 and =0 alternated, --repeats timed calls each after one warm-up call
          each, host clock around the call (upload, kernel, synchronisation), per value of --reach.
  text    --lines pairs of the first --inter as a twelve-column allValidPairs file: hicmi_ends_file, whole call.
The kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this script with --no-text.
Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
FORMS = (("combine", "0"), ("plain", "1"))


def main():
    from buildmap_bench import thinned
    from spans_bench import true_assembly
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--inter", default="0.02")
    ap.add_argument("--lines", type=int, default=3000000)
    ap.add_argument("--window", type=int, default=50000)
    ap.add_argument("--reach", default="2,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--no-text", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, supportEnds, synth

    reaches = [int(x) for x in args.reach.split(",")]
    lay0 = synth.make_layout(args.bins, seed=1)
    out = {"bins": args.bins, "window": args.window, "repeats": args.repeats, "cases": []}
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
        sizes = lay.scaffold_sizes_bp
        asm = true_assembly(lay)
        tables = (asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes)
        make_s = round(time.time() - t0, 1)
        for reach in reaches:
            rec = {"inter": inter, "reach": reach, "read_pairs_of_the_map": total, "pairs": int(len(pairs[0])),
                   "sequences": int(len(asm.seq_sizes)), "make_s": make_s}

            def count(flag, want=False):
                os.environ["HICMI_ENDS_PLAIN"] = flag
                with _lib.Context(0) as ctx:
                    ctx.ends_begin(sizes, *tables, args.window, reach)
                    ctx.synchronize()
                    t = time.perf_counter()
                    ctx.ends_add_pairs(*pairs)
                    dt = time.perf_counter() - t
                    return dt, ctx.ends_finish() if want else None
            results = {name: count(flag, want=True)[1] for name, flag in FORMS}     # warm-up, and the results
            times = {name: [] for name, _f in FORMS}
            for _k in range(args.repeats):
                for name, flag in FORMS:
                    times[name].append(count(flag)[0])
            os.environ.pop("HICMI_ENDS_PLAIN", None)
            table, counters = results["plain"]
            same = all(a.tobytes() == b.tobytes() for a, b in zip(results["plain"], results["combine"]))
            rec["count"] = {"same_bytes": bool(same), "counters": dict(zip(supportEnds.COUNTER_COLUMNS, counters.tolist())),
                            "placed": int(table.shape[0]), "counters_hit": int((table != 0).sum()), "largest_counter": int(table.max()),
                            "call_ms": {name: [round(v * 1e3, 3) for v in times[name]] for name in times},
                            "combine_slowest_beats_plain_fastest": bool(max(times["combine"]) < min(times["plain"]))}
            out["cases"].append(rec)
        del pairs

    if text_case is not None:
        lay, text_sample = text_case
        sizes, names = lay.scaffold_sizes_bp, lay.scaffold_names
        asm = true_assembly(lay)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "bench.allValidPairs")
            n_lines = synth.write_valid_pairs(path, lay, text_sample, seed=4, sort=True)
            rec = {"lines": n_lines, "file_MB": round(os.path.getsize(path) / 1e6, 1), "reach": reaches[0]}

            def drive(flag):
                os.environ["HICMI_ENDS_PLAIN"] = flag
                with _lib.Context(0) as ctx:
                    t = time.perf_counter()
                    stats = _lib.ends_file(path, names, sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, args.window,
                                           reaches[0], ctx, threads=args.threads)[0]
                    dt = time.perf_counter() - t
                assert stats[:4] == (n_lines, n_lines, 0, 0)
                return round(dt, 4)
            drive("0")                                                          # warm-up
            rec["ends_file_combine_s"] = [drive("0") for _k in range(args.repeats)]
            rec["ends_file_plain_s"] = [drive("1") for _k in range(args.repeats)]
            os.environ.pop("HICMI_ENDS_PLAIN", None)
            out["text"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
