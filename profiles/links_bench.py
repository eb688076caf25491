#!/usr/bin/env python3
"""The end-link graph on the device (hicmi_links_resident): the combining kernel against one find-or-insert
per pair, a links_resident call on the host clock with the share of its host sort, and a seats_resident call beside it.

    python profiles/links_bench.py [--bins 16000] [--pairs 8000000] [--inter 0.02] [--window 50000] [--every 4] [--repeats 3]
                                   [--forms combine,plain] [--out FILE]

The pairs are the ones profiles/pairs_bench.py draws, sorted as HiC-Pro sorts, on all scaffolds of the map (no ordering
takes part); all of them are loaded into one store, then Context.links_resident with the --forms alternated
(HICMI_LINKS_PLAIN=0 and =1), --repeats timed calls each after one warm-up call each, host clock around the call (sizes up,
two memsets, count, compact, records down, sort, merge, rows out), Context.links_info after each for the records, the slots
and the milliseconds of the sort, and as many Context.seats_resident calls on the layout seats_bench.py uses beside them.
The kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this script.  Prints one JSON object (and
writes it to --out).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))
ENV = {"combine": {"HICMI_LINKS_PLAIN": "0"}, "plain": {"HICMI_LINKS_PLAIN": "1"}}
KEYS = ("HICMI_LINKS_PLAIN",)


def set_form(name):
    for key in KEYS:
        os.environ.pop(key, None)
    if name:
        os.environ.update(ENV[name])


def main():
    from anchor_bench import without_every
    from buildmap_bench import thinned
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--inter", type=float, default=0.02)
    ap.add_argument("--window", type=int, default=50000)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forms", default="combine,plain")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, synth

    forms = args.forms.split(",")
    t0 = time.time()
    lay = synth.make_layout(args.bins, seed=1)
    counts, lay = synth.make_raw_counts(lay, seed=1, inter=args.inter)
    sample, total = thinned(counts, args.pairs, seed=2)
    del counts
    pairs = synth.draw_valid_pairs(lay, sample, seed=1, sort=True)
    del sample
    sizes, names = lay.scaffold_sizes_bp, lay.scaffold_names
    asm, _target = without_every(lay, args.every)
    tables = (asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes)
    n = int(len(pairs[0]))
    kept = int((pairs[0] != pairs[2]).sum())
    out = {"bins": args.bins, "window": args.window, "repeats": args.repeats, "scaffolds": len(names), "read_pairs_of_the_map": total,
           "pairs": n, "pairs_kept": kept, "slice": _lib.LINKS_SLICE, "lds_slots": _lib.LINKS_SLOTS,
           "library": os.path.basename(_lib.LIB_PATH), "make_s": round(time.time() - t0, 1)}

    def clock(call):
        t = time.perf_counter()
        got = call()
        return round((time.perf_counter() - t) * 1e3, 3), got

    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        results, times, sorts = {}, {form: [] for form in forms}, {form: [] for form in forms}
        for form in forms:                                                      # warm-up, and the results
            set_form(form)
            results[form] = ctx.links_resident(sizes, args.window)
        records, slots, _ms = ctx.links_info()
        ctx.seats_resident(sizes, *tables, args.window)
        seats_ms = []
        for _k in range(args.repeats):
            for form in forms:
                set_form(form)
                times[form].append(clock(lambda: ctx.links_resident(sizes, args.window))[0])
                sorts[form].append(round(ctx.links_info()[2], 3))
            seats_ms.append(clock(lambda: ctx.seats_resident(sizes, *tables, args.window))[0])
        set_form(None)
    lo, _hi, table, counters = results[forms[0]]
    out["count"] = {"links_resident_ms": times, "host_sort_ms": sorts, "seats_resident_ms": seats_ms, "records": records, "slots": slots,
                    "rows": int(len(lo)), "counters": [int(x) for x in counters],
                    "counters_sum_to_the_pairs_kept": bool(int(counters.sum()) == kept and int(table.sum()) == kept),
                    "forms_same_bytes": bool(all(all(a.tobytes() == b.tobytes() for a, b in zip(results[form], results[forms[0]]))
                                                 for form in forms))}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
