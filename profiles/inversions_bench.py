"""Inversion support and the refinement on bench.py's map: the synthetic map of --bins bins, seed 1,
after a resident -part1 -part2; one warm-up report, then the default path and HICMI_P2_INVERT_DIRECT=1 alternated,
--repeats each; the element reads counted by the host; the verdict counts; one refinement round and the rounds to
convergence from the bench ordering.  --reports N: only N default reports after the warm-up (for a kernel trace).

    python profiles/inversions_bench.py [--bins 16000] [--repeats 3] [--out FILE.json] [--reports N]
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
    ap.add_argument("--reports", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import torch
    from hic_genome_assembler_amd import orderGenome as p2, scaffoldToChromosomes as p1, synth
    from hic_genome_assembler_amd import _lib
    from hic_genome_assembler_amd.hostio import Bin
    os.environ.setdefault("HICMI_NO_PLOTS", "1")
    dev = torch.device("cuda", 0)
    lay = synth.make_layout(a.bins, seed=1)
    contacts = synth.dense_contacts_torch(lay, dev, seed=1, sinkhorn_iters=12)
    torch.cuda.synchronize()
    work = tempfile.mkdtemp(prefix="hicinv_")
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
    chromList, binList = dm.chromosome_groups, dm.kept_bins
    lengths = [[len(s.binList) for s in g] for g in ordered]

    def report(direct):
        os.environ.pop("HICMI_P2_INVERT_DIRECT", None)
        if direct:
            os.environ["HICMI_P2_INVERT_DIRECT"] = "1"
        t = time.perf_counter()
        res = p2.inversionSupport(matrix, ordered, binList, chromList)
        dt = time.perf_counter() - t
        os.environ.pop("HICMI_P2_INVERT_DIRECT", None)
        return dt, res

    report(False)                                             # warm-up
    if a.reports:
        for _ in range(a.reports):
            report(False)
        ctx.close()
        return
    times = {"default": [], "direct": []}
    res = {}
    for _ in range(a.repeats):
        for key in ("default", "direct"):
            dt, res[key] = report(key == "direct")
            times[key].append(dt)
    import numpy as np
    worst = 0.0
    for x, y in zip(res["default"], res["direct"]):
        m = np.asarray(y["table"]) != 0.0
        if m.any():
            worst = max(worst, float(np.max(np.abs(x["table"][m] - y["table"][m]) / np.abs(y["table"][m]))))
    rows = [r for x in res["default"] for r in x["rows"]]
    out = {
        "bins": a.bins, "chromosomes": len(ordered), "scaffolds": sum(len(g) for g in ordered),
        "largest_chromosome": {"bins": max(sum(ln) for ln in lengths), "scaffolds": max(len(ln) for ln in lengths)},
        "candidates_computed": sum(len(ln) * (len(ln) + 1) // 2 for ln in lengths),
        "element_reads_default": sum(p2.inversion_work(ln) for ln in lengths),
        "element_reads_direct": sum((len(ln) * (len(ln) + 1) // 2) * (sum(ln) * (sum(ln) - 1) // 2) for ln in lengths),
        "seconds_per_report": times,
        "largest_relative_difference_of_a_score": worst,
        "same_text": p2.inversionSupportText(res["default"]) == p2.inversionSupportText(res["direct"]),
        "verdicts": {v: sum(r["verdict"] == v for r in rows) for v in ("invertible", "supported", "NA")},
        "near_above_1": sum(r["near"] > 1 for r in rows),
        "largest_gains": sorted((r["gain"] for r in rows if r["gain"] is not None), reverse=True)[:5],
    }
    with contextlib.redirect_stdout(io.StringIO()):
        t = time.perf_counter()
        p2.refineOrdering(matrix, ordered, binList, chromList, maxRounds=1)
        out["one_refinement_round_s"] = time.perf_counter() - t
        t = time.perf_counter()
        _refined, log, summary = p2.refineOrdering(matrix, ordered, binList, chromList)
        out["refinement_s"] = time.perf_counter() - t
    out["refinement"] = {"moves": len(log), "by_kind": {k: sum(e["kind"] == k for e in log) for k in p2.REFINE_MOVES},
                         "rounds": max(s["rounds"] for s in summary), "converged": all(s["converged"] for s in summary),
                         "score_gain_relative": [(s["after"] - s["before"]) / s["before"] if s["before"] else 0.0 for s in summary]}
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
