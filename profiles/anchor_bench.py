#!/usr/bin/env python3
"""Anchoring on the device (hicmi_anchor_begin / _add_pairs / _finish / _file): the combining count kernel
against one atomic add per anchored pair, in sequence mode and in rank mode, and the one-pass driver on a text file.

    python profiles/anchor_bench.py [--bins 16000] [--pairs 8000000] [--inter 0.02] [--lines 3000000] [--window 50000]
                                    [--every 4] [--repeats 3] [--forms combine,plain] [--no-text] [--out FILE]

The pairs are the ones profiles/assembledmap_bench.py draws - the 16,000-bin make_raw_counts map thinned to about --pairs read
pairs, sorted as HiC-Pro sorts - and the assembly is the map's true layout with 100 bp between neighbours, from which every
--every-th scaffold of the size file is taken out: those are the candidates.  In rank mode every candidate has the
chromosome it was taken from as its target.
  count   Context.anchor_add_pairs, the --forms alternated (HICMI_ANCHOR_PLAIN=1 and =0), --repeats timed calls each after
          one warm-up call each, host clock around the call (upload, kernel, synchronisation), per mode.
  text    --lines pairs as a twelve-column allValidPairs file: hicmi_anchor_file in sequence mode, whole call.
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
ENV = {"combine": {"HICMI_ANCHOR_PLAIN": "0"}, "plain": {"HICMI_ANCHOR_PLAIN": "1"}}
KEYS = ("HICMI_ANCHOR_PLAIN",)


def set_form(name):
    for key in KEYS:
        os.environ.pop(key, None)
    if name:
        os.environ.update(ENV[name])


def without_every(lay, every):
    """(the true assembly without every ``every``-th scaffold of the size file, the target of each of those)."""
    from hic_genome_assembler_amd import assembledMap
    from spans_bench import GAP
    out = set(range(every - 1, len(lay.scaffold_names), every))
    groups = []
    for c in range(int(lay.scaffold_chrom.max()) + 1):
        members = sorted(np.flatnonzero(lay.scaffold_chrom == c).tolist(), key=lambda s: lay.scaffold_rank[s])
        groups.append([[lay.scaffold_names[s], "-" if lay.scaffold_orient[s] < 0 else "+"] for s in members if s not in out])
    asm = assembledMap.build_assembly(groups, lay.scaffold_names, lay.scaffold_sizes_bp, GAP, chromosomes_only=True)
    target = np.full(len(lay.scaffold_names), -1, np.int32)
    for s in out:
        target[s] = lay.scaffold_chrom[s]
    return asm, target


def main():
    from buildmap_bench import thinned
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
    ap.add_argument("--no-text", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, placeUnplaced, synth

    forms = args.forms.split(",")
    t0 = time.time()
    lay = synth.make_layout(args.bins, seed=1)
    counts, lay = synth.make_raw_counts(lay, seed=1, inter=args.inter)
    sample, total = thinned(counts, args.pairs, seed=2)
    text_sample = None if args.no_text else thinned(counts, args.lines, seed=3)[0]
    del counts
    pairs = synth.draw_valid_pairs(lay, sample, seed=1, sort=True)
    del sample
    sizes, names = lay.scaffold_sizes_bp, lay.scaffold_names
    asm, target = without_every(lay, args.every)
    tables = (asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes)
    out = {"bins": args.bins, "window": args.window, "every": args.every, "repeats": args.repeats, "scaffolds": len(names),
           "candidates": int((target >= 0).sum()), "sequences": int(len(asm.seq_sizes)), "read_pairs_of_the_map": total,
           "pairs": int(len(pairs[0])), "make_s": round(time.time() - t0, 1), "cases": []}
    for mode, tgt in (("sequence", None), ("rank", target)):
        def count(form, want=False):
            set_form(form)
            with _lib.Context(0) as ctx:
                ctx.anchor_begin(sizes, *tables, tgt, args.window)
                ctx.synchronize()
                t = time.perf_counter()
                ctx.anchor_add_pairs(*pairs)
                dt = time.perf_counter() - t
                return dt, ctx.anchor_finish() if want else None
        results = {form: count(form, want=True)[1] for form in forms}           # warm-up, and the results
        times = {form: [] for form in forms}
        for _k in range(args.repeats):
            for form in forms:
                times[form].append(count(form)[0])
        set_form(None)
        table, counters = results[forms[0]]
        same = all(a.tobytes() == b.tobytes() for form in forms[1:] for a, b in zip(results[forms[0]], results[form]))
        out["cases"].append({"mode": mode, "same_bytes": bool(same), "counters": dict(zip(placeUnplaced.COUNTER_COLUMNS, counters.tolist())),
                             "table": int(len(table)), "counters_hit": int((table != 0).sum()), "largest_counter": int(table.max()),
                             "call_ms": {form: [round(v * 1e3, 3) for v in times[form]] for form in forms}})
    del pairs

    if text_sample is not None:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "bench.allValidPairs")
            n_lines = synth.write_valid_pairs(path, lay, text_sample, seed=4, sort=True)
            rec = {"lines": n_lines, "file_MB": round(os.path.getsize(path) / 1e6, 1), "mode": "sequence"}

            def drive(form):
                set_form(form)
                with _lib.Context(0) as ctx:
                    t = time.perf_counter()
                    stats = _lib.anchor_file(path, names, sizes, *tables, None, args.window, ctx, threads=args.threads)[0]
                    dt = time.perf_counter() - t
                assert stats[:4] == (n_lines, n_lines, 0, 0)
                return round(dt, 4)
            drive(forms[0])                                                     # warm-up
            for form in forms:
                rec["anchor_file_%s_s" % form] = [drive(form) for _k in range(args.repeats)]
            set_form(None)
            out["text"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
