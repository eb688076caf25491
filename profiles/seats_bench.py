#!/usr/bin/env python3
"""Seat support on the device (hicmi_seats_resident): the combining kernel against up to four atomic adds per
pair, a seats_resident call against an anchor_resident call on the same store, and one relocate round of polishOrder.

    python profiles/seats_bench.py [--bins 16000] [--pairs 8000000] [--inter 0.02] [--lines 3000000] [--window 50000] [--every 4]
                                   [--repeats 3] [--forms combine,plain] [--no-polish] [--out FILE]

The pairs are the ones profiles/pairs_bench.py draws, sorted as HiC-Pro sorts, and the assembly is the one it makes: the
map's true layout without every --every-th scaffold of the size file.
  count   all pairs loaded into one store, then Context.seats_resident with the --forms alternated (HICMI_SEATS_PLAIN=0 and
          =1), --repeats timed calls each after one warm-up call each, host clock around the call (tables up, kernel, table
          down), and as many Context.anchor_resident calls in sequence mode beside them.
  polish  --lines pairs as a twelve-column allValidPairs file and the order file of the assembly with one scaffold per
          chromosome taken out and put back five places on: polishOrder -moves flip,relocate, every resident call and the
          whole run on the host clock.
The kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this script with --no-polish.  Prints one JSON
object (and writes it to --out).
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
ENV = {"combine": {"HICMI_SEATS_PLAIN": "0"}, "plain": {"HICMI_SEATS_PLAIN": "1"}}
KEYS = ("HICMI_SEATS_PLAIN",)


def set_form(name):
    for key in KEYS:
        os.environ.pop(key, None)
    if name:
        os.environ.update(ENV[name])


def main():
    from anchor_bench import without_every
    from buildmap_bench import thinned
    from pairs_bench import Clocked
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--inter", type=float, default=0.02)
    ap.add_argument("--lines", type=int, default=3000000)
    ap.add_argument("--window", type=int, default=50000)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forms", default="combine,plain")
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--no-polish", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, polishOrder, synth

    forms = args.forms.split(",")
    t0 = time.time()
    lay = synth.make_layout(args.bins, seed=1)
    counts, lay = synth.make_raw_counts(lay, seed=1, inter=args.inter)
    sample, total = thinned(counts, args.pairs, seed=2)
    text_sample = None if args.no_polish else thinned(counts, args.lines, seed=3)[0]
    del counts
    pairs = synth.draw_valid_pairs(lay, sample, seed=1, sort=True)
    del sample
    sizes, names = lay.scaffold_sizes_bp, lay.scaffold_names
    asm, _target = without_every(lay, args.every)
    tables = (asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes)
    n = int(len(pairs[0]))
    kept = int((pairs[0] != pairs[2]).sum())
    n_table = _lib.seats_blocks(sizes, asm.lift_seq, len(asm.seq_sizes))[1]
    out = {"bins": args.bins, "window": args.window, "every": args.every, "repeats": args.repeats, "scaffolds": len(names),
           "placed": _lib.ends_placed_count(sizes, asm.lift_seq), "sequences": int(len(asm.seq_sizes)), "table_counters": n_table,
           "read_pairs_of_the_map": total, "pairs": n, "pairs_kept": kept, "make_s": round(time.time() - t0, 1)}

    def clock(call):
        t = time.perf_counter()
        got = call()
        return round((time.perf_counter() - t) * 1e3, 3), got

    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        results, times = {}, {form: [] for form in forms}
        for form in forms:                                                      # warm-up, and the results
            set_form(form)
            results[form] = ctx.seats_resident(sizes, *tables, args.window)
        ctx.anchor_resident(sizes, *tables, None, args.window)
        anchor_ms = []
        for _k in range(args.repeats):
            for form in forms:
                set_form(form)
                times[form].append(clock(lambda: ctx.seats_resident(sizes, *tables, args.window))[0])
            anchor_ms.append(clock(lambda: ctx.anchor_resident(sizes, *tables, None, args.window))[0])
        set_form(None)
    first, table, counters = results[forms[0]]
    rec = {"seats_resident_ms": times, "anchor_resident_ms": anchor_ms, "counters": [int(x) for x in counters],
           "counters_sum_to_the_pairs": bool(int(counters.sum()) == n), "adds": int(table.sum()),
           "forms_same_bytes": bool(all(all(a.tobytes() == b.tobytes() for a, b in zip(results[form], results[forms[0]])) for form in forms)),
           "table_counters_used": int((table > 0).sum())}
    out["count"] = rec
    del pairs, results

    if text_sample is not None:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "bench.allValidPairs")
            n_lines = synth.write_valid_pairs(path, lay, text_sample, seed=4, sort=True)
            paths = {k: os.path.join(tmp, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
            with open(paths["hicProScaffSizeFile"], "w") as fh:
                fh.write("".join("%s\t%d\n" % ns for ns in zip(names, np.asarray(sizes).tolist())))
            order, displaced = os.path.join(tmp, "orders.txt"), 0
            with open(order, "w") as fh:
                for q, comps in enumerate(asm.components):
                    comps = list(comps)
                    if len(comps) > 12:
                        comps.insert(len(comps) // 2 + 5, comps.pop(len(comps) // 2))
                        displaced += 1
                    fh.write("### Chromosome grouping %d ###\n" % (q + 1))
                    fh.write("".join("%s\t%s\n" % (names[s], o) for s, _off, o in comps))
            cfg = synth.write_config(os.path.join(tmp, "config.txt"), paths, os.path.join(tmp, "save"), os.path.join(tmp, "plots"), 100000,
                                     extra={"validPairFile": path})
            with _lib.Context(0) as ctx:
                clocked = Clocked(ctx)
                t = time.perf_counter()
                status, rounds, log = polishOrder.main(["-config", cfg, "-order", order, "-window", str(args.window), "-moves", "flip,relocate",
                                                        "-out", os.path.join(tmp, "polished"), "-threads", str(args.threads)], context=clocked)
                dt = time.perf_counter() - t
            by_call = {}
            for name, ms in clocked.times:
                by_call.setdefault(name, []).append(ms)
            out["polish"] = {"lines": n_lines, "displaced": displaced, "status": status, "rounds": rounds,
                             "flips": sum(row[1] == "flip" for row in log), "relocations": sum(row[1] == "relocate" for row in log),
                             "whole_run_s": round(dt, 4), "calls": {name: len(v) for name, v in by_call.items()},
                             "call_ms_sum": {name: round(sum(v), 3) for name, v in by_call.items()},
                             "call_ms_median": {name: float(np.median(v)) for name, v in by_call.items()},
                             "s_per_round": round((dt - sum(by_call.get("pairs_file", [0])) / 1e3) / max(rounds, 1), 4)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
