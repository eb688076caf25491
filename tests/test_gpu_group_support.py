"""Group support on the GPU (k_group_support.hip through hicmi_group_sums) against the definition restated
in NumPy (tests/group_support_reference.py).  The summation order is part of the definition, so every table is compared
with ``==``: no tolerance anywhere in this file."""
import contextlib
import io
import os
import time

import numpy as np
import pytest

import golden_cases as gc
import group_support_reference as ref

pytestmark = pytest.mark.gpu

PLAIN = "HICMI_GROUP_SUPPORT_PLAIN"


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    monkeypatch.delenv(PLAIN, raising=False)


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _case(name):
    spec, _meta, _gold, lay, c = gc.load_case(name)
    bed = [(lay.scaffold_names[lay.scaffold_of_bin[k]], int(lay.bin_ids[k])) for k in range(lay.n_bins)]
    M, ids, scaffolds = ref.case_inputs(bed, c, [int(lay.bin_ids[b]) for b in spec.get("nan_bias", ())])
    groups = ref.read_group_file(os.path.join(gc.GOLDEN_DIR, name, "chromosomeGroups.txt"))
    return M, ids, scaffolds, groups, ref.scaffold_bin_counts(bed)


def _random_map(n, seed, zero_rows=()):
    rng = np.random.default_rng(seed)
    c = rng.random((n, n)) * (rng.random((n, n)) < 0.7)
    c = np.triu(c) + np.triu(c, 1).T
    for z in zero_rows:
        c[z, :] = 0.0
        c[:, z] = 0.0
    return np.ascontiguousarray(c)


def _scaffolds(n, seed, mean=6):
    """A dense scaffold id per bin: runs of random length, their ids shuffled."""
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < n:
        lens.append(int(rng.geometric(1.0 / mean)))
    lens[-1] -= sum(lens) - n
    ids = rng.permutation(len(lens))
    return np.repeat(ids, lens).astype(np.int32), len(lens)


def _check(ctx, M, grp, scaf, G, S, label):
    """Both tables of the default path, of a second call and of PLAIN against the reference, all with ==."""
    rb, rs = ref.group_sums(M, grp, scaf, G, S)
    b, s = ctx.group_sums(grp, scaf, G, S)
    b2, s2 = ctx.group_sums(grp, scaf, G, S)
    none, s3 = ctx.group_sums(grp, scaf, G, S, want_bins=False)
    os.environ[PLAIN] = "1"
    try:
        pb, ps = ctx.group_sums(grp, scaf, G, S)
    finally:
        del os.environ[PLAIN]
    print("%s: n %d, G %d, S %d, grouped rows %d; bin sums differing from the reference %d, scaffold sums %d; "
          "PLAIN %d / %d" % (label, len(M), G, S, int(np.count_nonzero(np.asarray(grp) >= 0)),
                             int(np.count_nonzero(b != rb)), int(np.count_nonzero(s != rs)),
                             int(np.count_nonzero(pb != rb)), int(np.count_nonzero(ps != rs))))
    assert np.array_equal(b, rb) and np.array_equal(s, rs)
    assert np.array_equal(b2, b) and np.array_equal(s2, s) and none is None and np.array_equal(s3, s)
    assert np.array_equal(pb, b) and np.array_equal(ps, s)
    return b, s


@pytest.mark.parametrize("name", gc.case_names())
def test_golden_cases_with_their_own_group_files(name):
    from hic_genome_assembler_amd import _lib
    M, ids, scaffolds, groups, counts = _case(name)
    sid = {s: k for k, s in enumerate(counts)}
    scaf = np.array([sid[s] for s in scaffolds], dtype=np.int32)
    grp = ref.labels_of(groups, ids).astype(np.int32)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M)
        _check(ctx, M, grp, scaf, len(groups), len(counts), name)


def test_label_and_shape_edges():
    """Random labels with -1 entries; G = 1; G = 300; a one-bin group; a scaffold that is the whole of its group (pairs 0,
    density 0.0); n = 1,237 (odd: the 8-byte form of the kernel, and not a tile multiple); no grouped row at all."""
    from hic_genome_assembler_amd import _lib
    n = 1237
    M = _random_map(n, 3, zero_rows=(5, 700))
    scaf, S = _scaffolds(n, 4)
    rng = np.random.default_rng(5)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M)
        grp = rng.integers(-1, 7, n).astype(np.int32)
        _check(ctx, M, grp, scaf, 7, S, "random labels")
        _check(ctx, M, np.where(rng.random(n) < 0.8, 0, -1).astype(np.int32), scaf, 1, S, "G = 1")
        _check(ctx, M, rng.integers(-1, 300, n).astype(np.int32), scaf, 300, S + 3, "G = 300, three scaffolds without a bin")
        grp = rng.integers(0, 3, n).astype(np.int32)
        grp[grp == 2] = -1
        grp[n - 1] = 2                                        # a one-bin group, the last (odd) column
        whole = int(scaf[100])
        grp[grp == 1] = -1
        grp[scaf == whole] = 1                                # group 1 is exactly one scaffold
        b, s = _check(ctx, M, grp, scaf, 3, S, "one-bin group, a scaffold that is its whole group")
        assert not s[whole, 1] and not b[scaf == whole, 1].any()
        b, s = _check(ctx, M, np.full(n, -1, np.int32), scaf, 2, S, "no grouped row")
        assert not b.any() and not s.any()
        with pytest.raises(_lib.HicmiError):
            ctx.group_sums(np.full(n, 2, np.int32), scaf, 2, S)
        with pytest.raises(_lib.HicmiError):
            ctx.group_sums(np.zeros(n, np.int32), np.full(n, S, np.int32), 2, S)
        with pytest.raises(_lib.HicmiError):
            ctx.group_sums(np.full(n, -2, np.int32), scaf, 2, S)


@pytest.mark.parametrize("n,ld", [(300, 320), (301, 320), (300, 333)])
def test_adopted_matrix_with_a_leading_dimension(n, ld):
    """ld > n: even n and ld (16-byte loads), odd n with an even ld (its last column is a lane of its own), odd ld (8-byte
    loads)."""
    import torch
    from hic_genome_assembler_amd import _lib
    M = _random_map(n, 7)
    scaf, S = _scaffolds(n, 8)
    grp = np.random.default_rng(9).integers(-1, 4, n).astype(np.int32)
    t = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda:0")
    t[:, :n] = torch.as_tensor(M, device="cuda:0")
    torch.cuda.synchronize()
    with _lib.Context(0) as ctx:
        ctx.set_contacts_device(t.data_ptr(), n, ld, keepalive=t)
        _check(ctx, M, grp, scaf, 4, S, "adopted n %d ld %d" % (n, ld))


def test_fp32_upload():
    from hic_genome_assembler_amd import _lib
    n = 640
    M32 = _random_map(n, 11).astype(np.float32)
    scaf, S = _scaffolds(n, 12)
    grp = np.random.default_rng(13).integers(-1, 5, n).astype(np.int32)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M32)
        _check(ctx, M32.astype(np.float64), grp, scaf, 5, S, "fp32 upload")


def _records_on_device(M, ids, scaffolds, groups, counts, compact):
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as p1
    from hic_genome_assembler_amd.hostio import Bin
    bins = [Bin(b, s, 0, 1, 1.0, 0.0) for b, s in zip(ids, scaffolds)]
    chroms = [[[int(ln.split("\t")[0]), ln.split("\t")[1]] for ln in lines] for _h, lines in groups]
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M)
        dm = p1.DeviceMatrix(ctx)
        if compact:
            dm, bins = _quiet(p1.removeRows, dm, bins, zeroRows=True, biasVals=False, store_row_sums=False)
        return p1.groupSupport(dm, bins, chroms, counts), ctx.n


KEYS = ("scaffold", "bins", "live_bins", "assigned", "best", "best_density", "second", "second_density", "ratio", "verdict",
        "runs", "live_ids", "density")


def test_zero_rows_before_and_after_compact():
    """n300_edges has three zero rows: the records of the uploaded map, of the compacted one and of the reference are
    the same."""
    M, ids, scaffolds, groups, counts = _case("n300_edges")
    kept, _gone = ref.withhold(groups, counts)
    exp = ref.records(M, ids, scaffolds, kept, counts)
    full, n_full = _records_on_device(M, ids, scaffolds, kept, counts, compact=False)
    small, n_small = _records_on_device(M, ids, scaffolds, kept, counts, compact=True)
    assert (n_full, n_small) == (298, 295)
    for got in (full, small):
        assert [[r[k] for k in KEYS] for r in got] == [[r[k] for k in KEYS] for r in exp]
    assert any(r["verdict"] == "rescued" for r in exp) and any(r["live_bins"] < r["bins"] for r in exp)


def _write_groups(path, groups):
    with open(path, "w") as fh:
        fh.write("".join(h + "\n" + "".join(ln + "\n" for ln in lines) for h, lines in groups))


@pytest.mark.parametrize("name", ["n300_edges", "n2000"])
def test_run_group_support_from_files(name, tmp_path):
    """runGroupSupport on the golden group file: the report is the reference module's text.  Then on the same file with
    every 5th scaffold withheld (but none that is the whole of its group): report and rescued file are the reference's,
    and a Part 2 run on the rescued file orders every rescued scaffold."""
    from hic_genome_assembler_amd import orderGenome as p2, supportPart1 as sp
    paths = _quiet(gc.write_case_files, name, str(tmp_path))
    spec = gc.load_case(name)[0]
    M, ids, scaffolds, groups, counts = _case(name)
    golden = os.path.join(gc.GOLDEN_DIR, name, "chromosomeGroups.txt")
    out, resc = str(tmp_path / "gs.txt"), str(tmp_path / "rescued.txt")
    got = _quiet(sp.runGroupSupport, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], golden, out,
                 rescuedFile=resc, fullDir=str(tmp_path / "full"))
    exp = ref.records(M, ids, scaffolds, groups, counts)
    with open(out) as fh:
        assert fh.read() == ref.report_text(exp)
    with open(resc) as fh, open(golden) as src:
        assert fh.read() == ref.rescued_text(exp, groups) == src.read()      # nothing to rescue: the input again
    assert [r["density"] for r in got] == [r["density"] for r in exp]
    with open(str(tmp_path / "full" / "groupSupport.full.tsv")) as fh:
        rows = fh.read().splitlines()
    assert rows[1:] == ["\t".join([r["scaffold"]] + [repr(v) for v in r["density"]]) for r in exp]

    kept, gone = ref.withhold(groups, counts)
    for g, (head, lines) in enumerate(kept):
        if not lines:                                         # a scaffold that was its whole group stays: Part 1 writes no
            kept[g] = groups[g]                               # empty group, and Part 2 does not order one
            gone = {s: h for s, h in gone.items() if h != g}
    assert all(lines for _h, lines in kept)
    held = str(tmp_path / "withheld.txt")
    _write_groups(held, kept)
    _quiet(sp.runGroupSupport, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], held, out,
           rescuedFile=resc)
    exp = ref.records(M, ids, scaffolds, kept, counts)
    with open(out) as fh:
        assert fh.read() == ref.report_text(exp)
    with open(resc) as fh:
        assert fh.read() == ref.rescued_text(exp, kept)
    rescued = [r for r in exp if r["verdict"] == "rescued"]
    print(name, "withheld %d, rescued %d" % (len(gone), len(rescued)))
    assert rescued and all(r["best"] == gone[r["scaffold"]] for r in rescued)
    chroms = _quiet(p2.readChromsFromFile, resc)
    for r in rescued:
        assert [e[0] for e in chroms[r["best"]] if e[1] == r["scaffold"]] == r["live_ids"]
    assert set(_quiet(p2.readGroupingsToValidBins, resc)) == {b for _h, lines in kept for b in (int(ln.split("\t")[0]) for ln in lines)} | \
        {b for r in rescued for b in r["live_ids"]}
    orders = str(tmp_path / "orders.txt")
    _quiet(p2.runPipeline, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], resc, orders,
           str(tmp_path), "synthetic", str(tmp_path / "g.png"), "t", str(tmp_path / "plotOrder.txt"), spec["n_scaffolds"],
           spec["scan_scaffolds"], 100000)
    with open(orders) as fh:
        ordered = [ln.split("\t")[0] for ln in fh.read().splitlines() if not ln.startswith("#")]
    assert len(ordered) == len(set(ordered))
    assert all(r["scaffold"] in ordered for r in rescued)
    still_out = [s for s in gone if s not in {r["scaffold"] for r in rescued}]
    assert not any(s in ordered for s in still_out)


def _part1_config(tmp_path, name, extra):
    from hic_genome_assembler_amd import synth
    spec, _meta, _gold, lay, _c = gc.load_case(name)
    paths = _quiet(gc.write_case_files, name, str(tmp_path))
    cfg = synth.write_config(str(tmp_path / "config.txt"), paths, str(tmp_path / "out"), str(tmp_path / "plots"),
                             lay.resolution, min_size=spec["min_size"], modularity=0.0, psig=spec["psig"],
                             n_scaffolds=spec["n_scaffolds"], scan_scaffolds=spec["scan_scaffolds"])
    with open(cfg, "a") as fh:
        fh.write("".join("%s = %s\n" % kv for kv in extra.items()))
    return cfg, str(tmp_path / "out")


@pytest.mark.parametrize("name", ["n300_edges", "n400_default"])
def test_part1_with_the_two_config_lines(name, tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as run
    cfg, out = _part1_config(tmp_path / "with", name, dict(groupSupportFile="groupSupport.txt",
                                                           rescuedChromosomeGroupFile="rescuedGroups.txt"))
    _quiet(run.main, ["-part1", "-part2", "-config", cfg])
    for fn in gc.OUTPUT_FILES:
        with open(os.path.join(out, fn)) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn
    M, ids, scaffolds, groups, counts = _case(name)
    exp = ref.records(M, ids, scaffolds, groups, counts)
    with open(os.path.join(out, "groupSupport.txt")) as fh:
        assert fh.read() == ref.report_text(exp)
    with open(os.path.join(out, "rescuedGroups.txt")) as fh:
        assert fh.read() == ref.rescued_text(exp, groups)
    # -part1 alone (the context is not kept for Part 2) writes them too; one line gives one file
    cfg, out = _part1_config(tmp_path / "one", name, dict(groupSupportFile="groupSupport.txt"))
    _quiet(run.main, ["-part1", "-config", cfg])
    with open(os.path.join(out, "groupSupport.txt")) as fh:
        assert fh.read() == ref.report_text(exp)
    assert not os.path.exists(os.path.join(out, "rescuedGroups.txt"))
    with open(os.path.join(out, "chromosomeGroups.txt")) as fh:
        assert fh.read() == gc.golden_text(name, "chromosomeGroups.txt")


def test_part1_without_the_lines_writes_no_new_file(tmp_path, capsys):
    from hic_genome_assembler_amd import run_hicAssembler as run
    name = "n160"
    cfg, out = _part1_config(tmp_path, name, {})
    run.main(["-part1", "-part2", "-config", cfg])
    printed = capsys.readouterr().out
    assert "Group support" not in printed and "rescued" not in printed
    assert not [fn for fn in os.listdir(out) if "upport" in fn or "escued" in fn]
    assert all(os.path.exists(os.path.join(out, fn)) for fn in gc.OUTPUT_FILES)
    for fn in gc.OUTPUT_FILES:
        with open(os.path.join(out, fn)) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn


def test_bench_map_of_16000_bins(tmp_path):
    """bench.py's map (16,000 bins, seed 1, sinkhorn_iters=12) adopted in device memory, the groups of a resident
    -part1: the default path against PLAIN with ==, both tables and every record; prints the seconds of both."""
    import torch
    from hic_genome_assembler_amd import _lib, scaffoldToChromosomes as p1, synth
    from hic_genome_assembler_amd.hostio import Bin
    n = 16000
    lay = synth.make_layout(n, seed=1)
    contacts = synth.dense_contacts_torch(lay, torch.device("cuda:0"), seed=1, sinkhorn_iters=12)
    torch.cuda.synchronize()
    bins = [Bin(int(lay.bin_ids[k]), lay.scaffold_names[lay.scaffold_of_bin[k]], int(lay.start[k]), int(lay.stop[k]), 1.0, 0.)
            for k in range(n)]
    counts = {}
    for b in bins:
        counts[b.chrom] = counts.get(b.chrom, 0) + 1
    sizes = str(tmp_path / "synth.sizes")
    with open(sizes, "w") as fh:
        fh.write("".join("%s\t%d\n" % (s, z) for s, z in zip(lay.scaffold_names, lay.scaffold_sizes_bp)))
    f = lambda k: str(tmp_path / k)  # noqa: E731
    with _lib.Context(0) as ctx:
        ctx.set_contacts_device(contacts.data_ptr(), n, keepalive=contacts)
        dm = p1.DeviceMatrix(ctx)
        _quiet(p1.runResident, dm, list(bins), sizes, f("dendrogramOrder.txt"), f("binGroups.txt"), f("assessment.txt"),
               f("chromosomeGroups.txt"), 5, 0.0, .05)
        groups = dm.chromosome_groups
        G, S = len(groups), len(counts)
        sid = {s: k for k, s in enumerate(counts)}
        label = {int(e[0]): g for g, grp in enumerate(groups) for e in grp}
        grp = np.array([label.get(b.ID, -1) for b in dm.kept_bins], dtype=np.int32)
        scaf = np.array([sid[b.chrom] for b in dm.kept_bins], dtype=np.int32)
        print("16k map: %d rows, %d groups, %d scaffolds, %d grouped rows" % (ctx.n, G, S, int((grp >= 0).sum())))
        seconds = {"default": [], "plain": []}
        tables, records = {}, {}
        for rep in range(3):
            for mode in ("default", "plain"):
                if mode == "plain":
                    os.environ[PLAIN] = "1"
                try:
                    t0 = time.perf_counter()
                    tables[mode] = ctx.group_sums(grp, scaf, G, S)
                    seconds[mode].append(time.perf_counter() - t0)
                    if rep == 0:
                        records[mode] = p1.groupSupport(dm, dm.kept_bins, groups, counts)
                finally:
                    os.environ.pop(PLAIN, None)
        print("16k map: seconds per group_sums call, default %s, PLAIN %s"
              % (["%.4f" % v for v in seconds["default"]], ["%.4f" % v for v in seconds["plain"]]))
        print("16k map: verdicts", ref.verdict_counts(records["default"]))
        assert np.array_equal(tables["default"][0], tables["plain"][0])
        assert np.array_equal(tables["default"][1], tables["plain"][1])
        assert records["default"] == records["plain"]
        assert tables["default"][1].any() and len(records["default"]) == S
