#!/usr/bin/env python3
"""The resident pair store on the device (hicmi_pairs_*, hicmi_ends_resident, hicmi_anchor_resident): the
stable compaction against one atomic bump per kept pair, the load of a text file against hicmi_ends_file, a resident call
against its file call, and polishOrder on a layout with scaffolds taken out and scaffolds turned round.

    python profiles/pairs_bench.py [--bins 16000] [--pairs 8000000] [--inter 0.02] [--lines 3000000] [--window 50000]
                                   [--every 4] [--flip-every 7] [--repeats 3] [--forms stable,plain] [--no-text] [--no-polish]
                                   [--out FILE]

The pairs are the ones profiles/anchor_bench.py draws, sorted as HiC-Pro sorts, and the assembly is the one it makes: the
map's true layout without every --every-th scaffold of the size file.
  keep    Context.pairs_add of all pairs into a fresh store, the --forms alternated (HICMI_PAIRS_PLAIN=0 and =1), --repeats
          timed calls each after one warm-up call each, host clock around the call (upload, kernels, synchronisation).
  text    --lines pairs as a twelve-column allValidPairs file: hicmi_pairs_file against hicmi_ends_file, whole calls; then on
          that store one hicmi_ends_resident and one hicmi_anchor_resident call against hicmi_ends_file / hicmi_anchor_file.
  polish  polishOrder on that file from the order file of the assembly with every --flip-every-th placed scaffold turned
          round: the load, every resident call and the whole run on the host clock.
The kernel times proper come from a `rocprofv3 --kernel-trace --stats` run of this script with --no-text --no-polish.
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
ENV = {"stable": {"HICMI_PAIRS_PLAIN": "0"}, "plain": {"HICMI_PAIRS_PLAIN": "1"}}
KEYS = ("HICMI_PAIRS_PLAIN",)


def set_form(name):
    for key in KEYS:
        os.environ.pop(key, None)
    if name:
        os.environ.update(ENV[name])


class Clocked:
    """A context of the library's whose store calls are timed on the host clock."""

    def __init__(self, ctx):
        self.ctx, self.times = ctx, []

    def __getattr__(self, name):
        call = getattr(self.ctx, name)

        def timed(*args, **kwargs):
            t = time.perf_counter()
            out = call(*args, **kwargs)
            self.times.append((name, round((time.perf_counter() - t) * 1e3, 3)))
            return out
        return timed


def main():
    from anchor_bench import without_every
    from buildmap_bench import thinned
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--pairs", type=int, default=8000000)
    ap.add_argument("--inter", type=float, default=0.02)
    ap.add_argument("--lines", type=int, default=3000000)
    ap.add_argument("--window", type=int, default=50000)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--flip-every", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--forms", default="stable,plain")
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--no-text", action="store_true")
    ap.add_argument("--no-polish", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from hic_genome_assembler_amd import _lib, polishOrder, synth

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
    n = int(len(pairs[0]))
    kept = int((pairs[0] != pairs[2]).sum())
    out = {"bins": args.bins, "window": args.window, "every": args.every, "repeats": args.repeats, "scaffolds": len(names),
           "candidates": int((target >= 0).sum()), "sequences": int(len(asm.seq_sizes)), "read_pairs_of_the_map": total,
           "pairs": n, "pairs_kept": kept, "share_kept": round(kept / max(n, 1), 4), "make_s": round(time.time() - t0, 1)}

    def keep(form, want=False):
        set_form(form)
        with _lib.Context(0) as ctx:
            ctx.pairs_begin(sizes)
            ctx.synchronize()
            t = time.perf_counter()
            ctx.pairs_add(*pairs)
            dt = time.perf_counter() - t
            if not want:
                return dt, None
            n_kept, n_intra, intra = ctx.pairs_info()
            return dt, (n_kept, n_intra, intra, ctx.pairs_fetch())
    results = {form: keep(form, want=True)[1] for form in forms}                # warm-up, and the results
    times = {form: [] for form in forms}
    for _k in range(args.repeats):
        for form in forms:
            times[form].append(keep(form)[0])
    set_form(None)
    want = tuple(a[pairs[0] != pairs[2]] for a in pairs)
    rec = {"call_ms": {form: [round(v * 1e3, 3) for v in times[form]] for form in forms}}
    for form in forms:
        n_kept, n_intra, intra, got = results[form]
        rec["%s_counts_right" % form] = bool(n_kept == kept and n_intra == n - kept
                                             and np.array_equal(intra, np.bincount(pairs[0][pairs[0] == pairs[2]], minlength=len(sizes))))
        rec["%s_store_is_the_mask" % form] = bool(all(np.array_equal(g, w) for g, w in zip(got, want)))
        if form == "plain":
            def rows(p):
                r = np.stack([np.asarray(x, np.int64) for x in p], axis=1)
                return r[np.lexsort(r.T[::-1])]
            rec["plain_same_multiset"] = bool(np.array_equal(rows(got), rows(want)))
    out["keep"] = rec
    del pairs, results, want

    if text_sample is not None:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "bench.allValidPairs")
            n_lines = synth.write_valid_pairs(path, lay, text_sample, seed=4, sort=True)
            rec = {"lines": n_lines, "file_MB": round(os.path.getsize(path) / 1e6, 1)}

            def clock(call):
                t = time.perf_counter()
                got = call()
                return round(time.perf_counter() - t, 4), got

            def load():
                with _lib.Context(0) as ctx:
                    dt, stats = clock(lambda: ctx.pairs_file(path, names, sizes, threads=args.threads))
                assert stats[:4] == (n_lines, n_lines, 0, 0)
                return dt

            def ends_file():
                with _lib.Context(0) as ctx:
                    return clock(lambda: _lib.ends_file(path, names, sizes, *tables, args.window, 2, ctx, threads=args.threads))[0]
            load()                                                              # warm-up
            ends_file()
            rec["pairs_file_s"], rec["ends_file_s"] = [], []
            for _k in range(args.repeats):
                rec["pairs_file_s"].append(load())
                rec["ends_file_s"].append(ends_file())
            with _lib.Context(0) as ctx:
                ctx.pairs_file(path, names, sizes, threads=args.threads)
                rec["pairs_kept"], rec["pairs_intra"] = ctx.pairs_info()[:2]
                ctx.ends_resident(sizes, *tables, args.window, 2)               # warm-up
                ctx.anchor_resident(sizes, *tables, None, args.window)
                rec["ends_resident_s"] = [clock(lambda: ctx.ends_resident(sizes, *tables, args.window, 2))[0] for _k in range(args.repeats)]
                rec["anchor_resident_s"] = [clock(lambda: ctx.anchor_resident(sizes, *tables, None, args.window))[0]
                                            for _k in range(args.repeats)]
                resident = ctx.ends_resident(sizes, *tables, args.window, 2), ctx.anchor_resident(sizes, *tables, None, args.window)
                rec["anchor_file_s"], from_file = clock(lambda: _lib.anchor_file(path, names, sizes, *tables, None, args.window, ctx,
                                                                                 threads=args.threads))
                ends_from_file = _lib.ends_file(path, names, sizes, *tables, args.window, 2, ctx, threads=args.threads)
                rec["resident_same_bytes"] = bool(all(a.tobytes() == b.tobytes() for a, b in zip(resident[0], ends_from_file[1:]))
                                                  and all(a.tobytes() == b.tobytes() for a, b in zip(resident[1], from_file[1:])))
            out["text"] = rec

            if not args.no_polish:
                paths = {k: os.path.join(tmp, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
                with open(paths["hicProScaffSizeFile"], "w") as fh:
                    fh.write("".join("%s\t%d\n" % ns for ns in zip(names, np.asarray(sizes).tolist())))
                order, k, flipped = os.path.join(tmp, "orders.txt"), 0, 0
                with open(order, "w") as fh:
                    for q, comps in enumerate(asm.components):
                        fh.write("### Chromosome grouping %d ###\n" % (q + 1))
                        for s, _off, o in comps:
                            k += 1
                            if k % args.flip_every == 0:
                                o, flipped = ("+" if o == "-" else "-"), flipped + 1
                            fh.write("%s\t%s\n" % (names[s], o))
                save = os.path.join(tmp, "save")
                cfg = synth.write_config(os.path.join(tmp, "config.txt"), paths, save, os.path.join(tmp, "plots"), 100000,
                                         extra={"validPairFile": path})
                with _lib.Context(0) as ctx:
                    clocked = Clocked(ctx)
                    dt, (status, rounds, log) = clock(lambda: polishOrder.main(["-config", cfg, "-order", order, "-window", str(args.window),
                                                                                "-out", os.path.join(tmp, "polished"),
                                                                                "-threads", str(args.threads)], context=clocked))
                by_call = {}
                for name, ms in clocked.times:
                    by_call.setdefault(name, []).append(ms)
                out["polish"] = {"turned_round": flipped, "taken_out": int((target >= 0).sum()), "status": status, "rounds": rounds,
                                 "flips": sum(row[1] == "flip" for row in log), "insertions": sum(row[1] == "place" for row in log),
                                 "whole_run_s": dt, "calls": {name: len(v) for name, v in by_call.items()},
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
