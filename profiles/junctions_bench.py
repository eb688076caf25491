"""Junction support on bench.py's map: the synthetic map of --bins bins, seed 1, after a resident
-part1 -part2; per window (16 and 0) one warm-up report, then the default path and HICMI_JUNCTIONS_PLAIN=1 alternated,
--repeats each; the records, workgroups and element reads counted by the host; the joins found and the chromosome count
after joining against the planted one.  --reports N: only N default reports per window after the warm-up (for a kernel
trace).

    python profiles/junctions_bench.py [--bins 16000] [--repeats 3] [--windows 16,0] [--out FILE.json] [--reports N]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=16000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--windows", type=str, default="16,0")
    ap.add_argument("--reports", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from hic_genome_assembler_amd import orderGenome as p2, scaffoldToChromosomes as p1, synth
    from hic_genome_assembler_amd import _lib
    from hic_genome_assembler_amd.hostio import Bin
    os.environ.setdefault("HICMI_NO_PLOTS", "1")
    dev = torch.device("cuda", 0)
    lay = synth.make_layout(a.bins, seed=1)
    contacts = synth.dense_contacts_torch(lay, dev, seed=1, sinkhorn_iters=12)
    torch.cuda.synchronize()
    work = tempfile.mkdtemp(prefix="hicjn_")
    f = lambda k: os.path.join(work, k)
    bench.write_sizes(lay, f("synth.sizes"))
    ctx = _lib.Context(0)
    bins = bench.make_bins(lay, Bin)
    ctx.set_contacts_device(contacts.data_ptr(), a.bins, keepalive=contacts)
    dm = p1.DeviceMatrix(ctx)
    with contextlib.redirect_stdout(io.StringIO()):
        p1.runResident(dm, list(bins), f("synth.sizes"), f("dendrogramOrder.txt"), f("binGroups.txt"), f("assessment.txt"),
                       f("chromosomeGroups.txt"), 5, 0.0, .05, overlap_files=True)
        matrix = p2.GenomeMatrix(ctx)
        ordered = p2.runResident(matrix, dm.kept_bins, f("chromosomeGroups.txt"), f("chromosomeOrders.txt"), f("plotOrder.txt"),
                                 6, 5, lay.resolution, chromosomeList=dm.chromosome_groups,
                                 on_native_phase=dm.release_files)
        dm.finish_files()
    binList = dm.kept_bins

    def report(window, plain):
        os.environ.pop("HICMI_JUNCTIONS_PLAIN", None)
        if plain:
            os.environ["HICMI_JUNCTIONS_PLAIN"] = "1"
        t = time.perf_counter()
        res = p2.junctionSupport(matrix, ordered, binList, window=window)
        dt = time.perf_counter() - t
        os.environ.pop("HICMI_JUNCTIONS_PLAIN", None)
        return dt, res

    out = {"bins": a.bins, "chromosomes": len(ordered), "scaffolds": sum(len(g) for g in ordered),
           "planted_chromosomes": len(set(lay.chrom_of_bin.tolist())), "windows": {}}
    for window in [int(w) for w in a.windows.split(",")]:
        report(window, False)                                 # warm-up
        if a.reports:
            for _ in range(a.reports):
                report(window, False)
            continue
        times = {"default": [], "plain": []}
        res = {}
        for _ in range(a.repeats):
            for key in ("default", "plain"):
                dt, res[key] = report(window, key == "plain")
                times[key].append(dt)
        rec = res["default"]["rec"]
        joined = p2.join_chromosomes(p2._plain(ordered), res["default"]["joinable"])[0]
        rels = sorted(r["rel"] for r in res["default"]["internal"] if r["rel"] is not None)
        out["windows"][str(window)] = {
            "records": int(len(rec)), "internal_junctions": len(res["default"]["internal"]),
            "workgroups": int(np.sum((rec[:, 2] + 63) // 64)), "element_reads": int(np.sum(rec[:, 2] * rec[:, 5])),
            "largest_record": [int(v) for v in rec[np.argmax(rec[:, 2] * rec[:, 5])][[2, 5]]],
            "seconds_per_report": times,
            "largest_relative_difference_of_a_sum": float(np.max(np.abs(res["default"]["sums"] - res["plain"]["sums"])
                                                                 / res["plain"]["sums"])),
            "same_picks": [r["best"] for r in res["default"]["ends"]] == [r["best"] for r in res["plain"]["ends"]],
            "ref": res["default"]["ref"], "joins": len(res["default"]["joinable"]), "weak": len(res["default"]["weak"]),
            "chromosomes_after_joining": len(joined),
            "smallest_rel_of_a_join": min([r["rel"] for r in res["default"]["ends"] if r["verdict"] == "joinable"] or [None]),
            "largest_rel_of_a_free_end": max([r["rel"] for r in res["default"]["ends"] if r["verdict"] == "free"] or [None]),
            "smallest_internal_rel": rels[:3],
        }
    ctx.close()
    if a.reports:
        return
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
