#!/usr/bin/env python3
"""Spanning depth on the device (hicmi_span_begin / _add_pairs / _finish / _file): the combining mark kernel
against two atomic adds per pair, the scans and picks at the cell count of the bench assembly, and the one-pass driver on a
text file.

    python profiles/spans_bench.py [--bins 16000] [--pairs 8000000] [--inter 0.02,0.0002] [--lines 3000000] [--step 10000]
                                   [--flank 8] [--repeats 3] [--no-text] [--out FILE]

The pairs are the ones profiles/assembledmap_bench.py draws - the 16,000-bin make_raw_counts map thinned to about --pairs read
pairs, sorted as HiC-Pro sorts, per value of --inter - and the assembly is the map's true layout with 100 bp between
neighbours, cut into cells of --step bp.
  mark    Context.span_add_pairs, HICMI_SPANS_PLAIN=1 and =0 alternated, --repeats timed calls each after one warm-up call
          each, host clock around the call (upload, kernel, synchronisation).
  finish  Context.span_finish with the records of a supportSpans report: two scans, the picks, the downloads.
  text    --lines pairs of the first --inter as a twelve-column allValidPairs file: hicmi_span_file, whole call.
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
GAP = 100


def true_assembly(lay):
    """The planted chromosomes as an assembledMap.Assembly."""
    from hic_genome_assembler_amd import assembledMap
    groups = []
    for c in range(int(lay.scaffold_chrom.max()) + 1):
        members = sorted(np.flatnonzero(lay.scaffold_chrom == c).tolist(), key=lambda s: lay.scaffold_rank[s])
        groups.append([[lay.scaffold_names[s], "-" if lay.scaffold_orient[s] < 0 else "+"] for s in members])
    return assembledMap.build_assembly(groups, lay.scaffold_names, lay.scaffold_sizes_bp, GAP)


def main():
    from buildmap_bench import thinned
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--inter", default="0.02,0.0002")
    ap.add_argument("--lines", type=int, default=3000000)
    ap.add_argument("--step", type=int, default=10000)
    ap.add_argument("--flank", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--no-text", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, supportSpans, synth

    lay0 = synth.make_layout(args.bins, seed=1)
    out = {"bins": args.bins, "step": args.step, "flank": args.flank, "repeats": args.repeats, "gap": GAP, "cases": []}
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
        cell_first, seq_first = supportSpans.number_cells(asm, sizes, args.step)
        recs, of_scaffold, of_junction = supportSpans.make_records(asm, sizes, args.step, cell_first, seq_first)
        rec = {"inter": inter, "read_pairs_of_the_map": total, "pairs": int(len(pairs[0])), "sequences": int(len(asm.seq_sizes)),
               "cells": int(seq_first[-1]), "records": int(len(recs)), "make_s": round(time.time() - t0, 1)}

        def mark(flag, want=False):
            os.environ["HICMI_SPANS_PLAIN"] = flag
            with _lib.Context(0) as ctx:
                ctx.span_begin(sizes, *tables, args.step)
                ctx.synchronize()
                t = time.perf_counter()
                ctx.span_add_pairs(*pairs)
                dt = time.perf_counter() - t
                if not want:
                    return dt, None
                t = time.perf_counter()
                got = ctx.span_finish(args.flank, recs)
                return dt, got + (time.perf_counter() - t,)
        results = {name: mark(flag, want=True)[1] for name, flag in FORMS}     # warm-up, and the results
        times = {name: [] for name, _f in FORMS}
        for _k in range(args.repeats):
            for name, flag in FORMS:
                times[name].append(mark(flag)[0])
        finish_ms = []
        for _k in range(args.repeats):
            finish_ms.append(round(mark("0", want=True)[1][3] * 1e3, 3))
        os.environ.pop("HICMI_SPANS_PLAIN", None)
        picks, counters, depth, _dt = results["plain"]
        same = all(a.tobytes() == b.tobytes() for a, b in zip(results["plain"][:3], results["combine"][:3]))
        marks = np.diff(np.concatenate([[0], depth.astype(np.int64)]))
        rec["mark"] = {"same_bytes": bool(same), "counters": dict(zip(supportSpans.COUNTER_COLUMNS, counters.tolist())),
                       "slots_marked": int(np.count_nonzero(marks)), "largest_depth": int(depth.max()),
                       "call_ms": {name: [round(v * 1e3, 3) for v in times[name]] for name in times},
                       "combine_slowest_beats_plain_fastest": bool(max(times["combine"]) < min(times["plain"]))}
        rec["finish"] = {"call_ms": finish_ms, "picks_competing": int((picks[:, 0] >= 0).sum())}
        out["cases"].append(rec)
        del pairs

    if text_case is not None:
        lay, text_sample = text_case
        sizes, names = lay.scaffold_sizes_bp, lay.scaffold_names
        asm = true_assembly(lay)
        cell_first, seq_first = supportSpans.number_cells(asm, sizes, args.step)
        recs = supportSpans.make_records(asm, sizes, args.step, cell_first, seq_first)[0]
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "bench.allValidPairs")
            n_lines = synth.write_valid_pairs(path, lay, text_sample, seed=4, sort=True)
            rec = {"lines": n_lines, "file_MB": round(os.path.getsize(path) / 1e6, 1)}

            def drive(flag):
                os.environ["HICMI_SPANS_PLAIN"] = flag
                with _lib.Context(0) as ctx:
                    t = time.perf_counter()
                    stats = _lib.span_file(path, names, sizes, asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes, args.step, 0,
                                           args.flank, recs, ctx, threads=args.threads)[0]
                    dt = time.perf_counter() - t
                assert stats[:4] == (n_lines, n_lines, 0, 0)
                return round(dt, 4)
            drive("0")                                                          # warm-up
            rec["span_file_combine_s"] = [drive("0") for _k in range(args.repeats)]
            rec["span_file_plain_s"] = [drive("1") for _k in range(args.repeats)]
            os.environ.pop("HICMI_SPANS_PLAIN", None)
            out["text"] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
