#!/usr/bin/env python3
"""The end-link graph on lifted ends on the device (hicmi_links_lifted): the combining kernel against one
find-or-insert per pair, on the layout anchor_bench.without_every gives and on identity tables, with links_resident calls on
the same store in the same run beside them - what the lift costs.

    python profiles/links_lifted_bench.py [--bins 16000] [--pairs 8000000] [--inter 0.02] [--window 50000] [--every 4]
                                          [--repeats 3] [--forms combine,plain] [--out FILE]

The pairs are the ones profiles/links_bench.py draws, sorted as HiC-Pro sorts; all of them are loaded into one store, then
per repeat and form (HICMI_LINKS_PLAIN=0 and =1) one Context.links_lifted call per layout and one Context.links_resident
call, after one warm-up call each, host clock around the call (tables up, two memsets, count, compact, records down, sort,
merge, rows out).  The kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this script.  Prints one
JSON object (and writes it to --out).
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


def set_form(name):
    os.environ.pop("HICMI_LINKS_PLAIN", None)
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
    import numpy as np
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
    n_scaf = len(names)
    layouts = {"without_every": (asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes),
               "identity": (np.arange(n_scaf, dtype=np.int32), np.zeros(n_scaf, np.int64), np.zeros(n_scaf, np.uint8),
                            np.asarray(sizes, np.int64))}
    kept = int((pairs[0] != pairs[2]).sum())
    out = {"bins": args.bins, "window": args.window, "repeats": args.repeats, "scaffolds": n_scaf, "read_pairs_of_the_map": total,
           "pairs": int(len(pairs[0])), "pairs_kept": kept, "slice": _lib.LINKS_SLICE, "lds_slots": _lib.LINKS_SLOTS,
           "sequences": {name: int(len(t[3])) for name, t in layouts.items()},
           "library": os.path.basename(_lib.LIB_PATH), "make_s": round(time.time() - t0, 1)}

    def clock(call):
        t = time.perf_counter()
        got = call()
        return round((time.perf_counter() - t) * 1e3, 3), got

    calls = {name: (lambda ctx, t=t: ctx.links_lifted(sizes, *t, args.window)) for name, t in layouts.items()}
    calls["links_resident"] = lambda ctx: ctx.links_resident(sizes, args.window)
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        results, info = {}, {}
        times = {what: {form: [] for form in forms} for what in calls}
        for form in forms:                                                      # warm-up, and the results
            set_form(form)
            for what, call in calls.items():
                results[what, form] = call(ctx)
                info[what] = ctx.links_info()[:2]
        for _k in range(args.repeats):
            for form in forms:
                set_form(form)
                for what, call in calls.items():
                    times[what][form].append(clock(lambda: call(ctx))[0])
        set_form(None)
    out["count"] = {}
    for what in calls:
        lo, _hi, table, counters = results[what, forms[0]]
        same = all(all(a.tobytes() == b.tobytes() for a, b in zip(results[what, form], results[what, forms[0]])) for form in forms)
        out["count"][what] = {"call_ms": times[what], "records": info[what][0], "slots": info[what][1], "rows": int(len(lo)),
                              "counters": [int(x) for x in counters], "counters_sum_to_the_pairs_kept": bool(int(counters.sum()) == kept),
                              "rows_sum_to_linked_plus_middle": bool(int(table.sum()) == int(counters[:2].sum())),
                              "forms_same_bytes": bool(same)}
    ident, flat = results["identity", forms[0]], results["links_resident", forms[0]]
    out["identity_rows_are_the_scaffold_rows"] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(ident[:3], flat[:3])))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
