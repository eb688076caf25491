"""Part 2's batched native calls against the per-chromosome path they replace.

* hicmi_p2_start_all (the start phase of every chromosome in one call) against hicmi_p2_select / _layout /
  _set_arrangement / _arrangement_total / _window_tables / _decide_window per chromosome: totals, winning candidates
  and literal costs with ``==`` on the doubles, then orderGenome with HICMI_PART2_START_ALL on and off: the same
  brute-force order and orientations, the same printed lines, the same files.
* hicmi_p2_scan_arranged (the scan entered with the insertion's ids / rev) against scanOrdering's path through Scaffold
  objects.

Nothing here is a tolerance: the batched calls run the same kernels on the same operands in the same order within a
chromosome, so every comparison is equality.
"""
import contextlib
import io
import os
import types

import numpy as np
import pytest

import golden_cases as gc

pytestmark = pytest.mark.gpu

P2_FILES = ("chromosomeOrders.txt", "plotOrder.txt")


@pytest.fixture(scope="module")
def hic():
    from hic_genome_assembler_amd import _lib
    _lib.load()
    return _lib


def _bin_objects(n):
    return [types.SimpleNamespace(ID=i + 1) for i in range(n)]


def _groups_from_lengths(chroms):
    """chroms: per chromosome the bin counts of its scaffolds, laid out one after the other along the matrix.  Returns
    (chromList as readChromsFromFile gives it, number of bins)."""
    out, b = [], 0
    for c, lens in enumerate(chroms):
        rows = []
        for s, ln in enumerate(lens):
            rows += [[b + e + 1, "c%d_s%d" % (c, s)] for e in range(ln)]
            b += ln
        out.append(rows)
    return out, b


def _decay_map(n, seed, blocks=()):
    """Symmetric positive contacts that fall off with distance plus noise; ``blocks``: (first, last) bin ranges whose
    contacts with everything, themselves included, are exactly zero."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    c = 1000.0 / (1.0 + np.abs(i[:, None] - i[None, :])) ** 0.9 * rng.uniform(0.5, 1.5, (n, n))
    c = (c + c.T) / 2
    for a, b in blocks:
        c[a:b, :] = 0.0
        c[:, a:b] = 0.0
    return np.ascontiguousarray(c)


def _flags(monkeypatch, p2, start_all, scan_arranged):
    monkeypatch.setattr(p2, "START_ALL", start_all)
    monkeypatch.setattr(p2, "SCAN_ARRANGED", scan_arranged)


def _drop_clock(text):
    return [ln for ln in text.splitlines() if not ln.startswith("RunTime for total genome")]


def _order_genome(hic, p2, contacts, chromList, n_scaffolds, scan_scaffolds, tmp, device_ptr=None):
    """One orderGenome + the two Part 2 files on a fresh context: (outcome, stdout lines, file texts).  The outcome is
    the ordering as (name, orientation, bins) triples, or the error it ended with."""
    os.makedirs(tmp, exist_ok=True)
    n = len(contacts) if device_ptr is None else device_ptr[1]
    bins = _bin_objects(n)
    files = [os.path.join(tmp, k) for k in P2_FILES]
    buf = io.StringIO()
    with hic.Context(0) as ctx:
        if device_ptr is None:
            ctx.set_contacts(contacts)
        else:
            ctx.set_contacts_device(device_ptr[0], n, keepalive=device_ptr[2])
        try:
            with contextlib.redirect_stdout(buf):
                ordered = p2.runResident(p2.GenomeMatrix(ctx), bins, None, files[0], files[1], n_scaffolds, scan_scaffolds,
                                         100000, chromosomeList=chromList)
            outcome = [[(s.name, s.orientation, list(s.binList)) for s in group] for group in ordered]
            texts = [open(k).read() for k in files]
        except (RuntimeError, hic.HicmiError) as e:
            outcome, texts = ("error", type(e).__name__, str(e)), None
    return outcome, _drop_clock(buf.getvalue()), texts


def _start_phase(lines):
    """The lines up to the last one the start phase prints: they come from the calling thread, in a fixed order."""
    marks = ("Initial permutations", "WARNING/ERROR", "Scaffolds to order")
    last = max((i for i, ln in enumerate(lines) if ln.startswith(marks)), default=-1)
    return lines[:last + 1]


def _same_runs(a, b):
    assert a[0] == b[0]
    assert _start_phase(a[1]) == _start_phase(b[1])
    assert sorted(a[1]) == sorted(b[1])                    # (the scan threads' blocks may interleave)
    assert a[2] == b[2]


# ------------------------------------------------------------------------------------------ the native call itself
def _start_one_by_one(p2, ctx, job, n_scaffolds):
    """What _startChromosome asks of the library for one chromosome: (total, pick, cost, status) as p2_start_all reports."""
    _ctx, sel, start, length, first = job
    ctx.p2_select(sel)
    ctx.p2_layout(start, length)
    k = len(first)
    if sum(length[i] for i in first) < 2:
        return 0.0, -1, 0.0, 1
    ctx.p2_set_arrangement(first, np.zeros(k, np.uint8))
    total = ctx.p2_arrangement_total()
    if total == 0:
        return total, -1, 0.0, 1
    ctx.p2_window_tables(*p2._table_arrays(k))
    pick, cost, _pf = ctx.p2_decide_window(0, k, total, 0., None)
    return (total, pick, cost, 0) if pick >= 0 else (total, -1, 0.0, 2)


def _jobs(p2, ctx, chromList, n, n_scaffolds, order):
    gm = p2.GenomeMatrix(ctx)
    bins = _bin_objects(n)
    gm.bin_index(bins)
    lanes = [gm] + [p2.GenomeMatrix(c) for c in ctx.workers(len(chromList) - 1)]
    for m in lanes[1:]:
        m._bin_index, m._bin_index_src = gm._bin_index, gm._bin_index_src
    lanes = dict(zip(range(len(chromList)), lanes))
    with contextlib.redirect_stdout(io.StringIO()):
        prepared, jobs = p2._startJobs(order, chromList, lanes, bins, n_scaffolds)
    return lanes, prepared, jobs


MIXED = [[5], [40, 30, 20], [6, 5, 4, 3, 3, 2, 2], [1], [30, 25, 22, 20, 18, 15, 12, 10, 8, 6, 5, 3, 2, 1, 1],
         [50, 3], [14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 1, 1, 1, 1, 1, 1], [1, 1, 1]]
MIXED_ZERO = 2              # the chromosome whose contacts are all zero


def _mixed():
    chromList, n = _groups_from_lengths(MIXED)
    first = sum(sum(c) for c in MIXED[:MIXED_ZERO])
    return chromList, n, _decay_map(n, 5, blocks=[(first, first + sum(MIXED[MIXED_ZERO]))])


@pytest.mark.parametrize("n_scaffolds", [6, 8, 3])
@pytest.mark.parametrize("order", ["largest-first", "smallest-first"])
def test_start_all_equals_the_calls_it_replaces(hic, n_scaffolds, order):
    """One call over a genome that mixes a chromosome of one scaffold, one of one bin, chromosomes with fewer than
    nScaffolds scaffolds (their own k), one without contacts (status 1) and ordinary ones - in both job orders, so that
    the shared H table is first taken by a small and by a large chromosome: every output of every job ``==`` what the
    per-chromosome calls give on a context of their own, and a second call on the same contexts gives the same again."""
    from hic_genome_assembler_amd import orderGenome as p2
    chromList, n, contacts = _mixed()
    todo = sorted(range(len(chromList)), key=lambda i: len(chromList[i]), reverse=order == "largest-first")
    with hic.Context(0) as ctx:
        ctx.set_contacts(contacts)
        lanes, _prepared, jobs = _jobs(p2, ctx, chromList, n, n_scaffolds, todo)
        tables = {k: p2._table_arrays(k) for k in {len(j[4]) for j in jobs}}
        assert len(tables) > 1                                   # several k in ONE call
        got = ctx.p2_start_all(jobs, tables)
        again = ctx.p2_start_all(jobs, tables)
        with hic.Context(0) as ref_ctx:
            ref_ctx.set_contacts(contacts)
            want = [_start_one_by_one(p2, ref_ctx, job, n_scaffolds) for job in jobs]
    assert [w[3] for w in want].count(1) == 2 and [w[3] for w in want].count(0) == len(want) - 2
    assert want[todo.index(MIXED_ZERO)][3] == 1 and want[todo.index(MIXED_ZERO)][0] == 0.0
    for g, a, w in zip(got, again, want):
        assert g == w and a == w                                 # tuples of floats and ints: == on the doubles


def test_start_all_with_short_lists_from_the_device_and_from_the_host(hic, monkeypatch):
    """k = 7 and 8 take the device short lists (k_win_near), smaller k the downloaded deltas: both inside one call."""
    from hic_genome_assembler_amd import orderGenome as p2
    chroms = [[9, 8, 7, 6, 5, 4, 3, 2, 2], [12, 10, 9, 7, 5, 4, 3], [20, 10, 5, 4], [6, 6, 6, 6, 6, 6, 6, 6, 1, 1]]
    chromList, n = _groups_from_lengths(chroms)
    contacts = _decay_map(n, 11)
    todo = list(range(len(chroms)))
    with hic.Context(0) as ctx:
        ctx.set_contacts(contacts)
        _lanes, _prepared, jobs = _jobs(p2, ctx, chromList, n, 8, todo)
        assert sorted(len(j[4]) for j in jobs) == [4, 7, 8, 8]
        got = ctx.p2_start_all(jobs, {k: p2._table_arrays(k) for k in (4, 7, 8)})
        with hic.Context(0) as ref_ctx:
            ref_ctx.set_contacts(contacts)
            want = [_start_one_by_one(p2, ref_ctx, job, 8) for job in jobs]
    assert got == want and all(w[3] == 0 for w in want)


def test_start_all_reports_bad_jobs(hic):
    from hic_genome_assembler_amd import orderGenome as p2
    chromList, n = _groups_from_lengths([[4, 3, 2], [5, 5]])
    with hic.Context(0) as ctx:
        ctx.set_contacts(_decay_map(n, 3))
        _lanes, _prepared, jobs = _jobs(p2, ctx, chromList, n, 6, [0, 1])
        with pytest.raises(hic.HicmiError):
            ctx.p2_start_all(jobs, {3: p2._table_arrays(3)})                       # no tables for k = 2
        with pytest.raises(hic.HicmiError):
            ctx.p2_start_all([jobs[0], jobs[0]], {3: p2._table_arrays(3)})         # one context twice
        bad = (jobs[1][0], [0, 1, n + 5], [0, 2], [2, 1], [0, 1])
        with pytest.raises(hic.HicmiError):
            ctx.p2_start_all([jobs[0], bad], {3: p2._table_arrays(3), 2: p2._table_arrays(2)})
        tables = {3: p2._table_arrays(3), 2: p2._table_arrays(2)}
        assert [r[3] for r in ctx.p2_start_all(jobs, tables)] == [0, 0]            # the contexts are usable afterwards


# ------------------------------------------------------------------------------------------ through orderGenome
@pytest.mark.parametrize("n_scaffolds,scan_scaffolds", [(6, 5), (9, 5), (3, 3)])
def test_mixed_genome_both_ways(hic, monkeypatch, tmp_path, n_scaffolds, scan_scaffolds):
    """orderGenome on the mixed genome with the batched start and with the per-chromosome start: the same ordering (or
    the same error), the same printed lines, the same two files.  nScaffolds = 9 is clipped to 8 with its line printed
    per chromosome."""
    from hic_genome_assembler_amd import orderGenome as p2
    chromList, n, contacts = _mixed()
    runs = []
    for k, (start_all, scan_arranged) in enumerate([(True, True), (False, False), (True, False), (False, True)]):
        _flags(monkeypatch, p2, start_all, scan_arranged)
        runs.append(_order_genome(hic, p2, contacts, chromList, n_scaffolds, scan_scaffolds, str(tmp_path / str(k))))
    for other in runs[1:]:
        _same_runs(runs[0], other)
    if n_scaffolds == 9:
        assert runs[0][1].count("Number of initial scaffolds to order by brute force method is set too high... setting it to 8") \
            == len(chromList)


def test_second_ordering_on_the_same_contexts(hic, monkeypatch, tmp_path):
    """The state hicmi_p2_start_all and hicmi_p2_scan_arranged leave in the contexts is reusable: two genomes ordered one
    after the other on the same context and workers, the second with fewer and smaller chromosomes, both ways."""
    from hic_genome_assembler_amd import orderGenome as p2
    chromList, n, contacts = _mixed()
    keep = [i for i in range(len(chromList)) if i != MIXED_ZERO]
    first = [chromList[i] for i in keep]
    second = [chromList[i] for i in reversed(keep[2:])]
    bins = _bin_objects(n)
    results = {}
    for flag in (True, False):
        _flags(monkeypatch, p2, flag, flag)
        with hic.Context(0) as ctx:
            ctx.set_contacts(contacts)
            gm = p2.GenomeMatrix(ctx)
            with contextlib.redirect_stdout(io.StringIO()):
                a = p2.orderGenome(gm, first, bins, 100000, 6, 5, plotChrom=False)
                b = p2.orderGenome(gm, second, bins, 100000, 4, 4, plotChrom=False)
        results[flag] = [[[(s.name, s.orientation, list(s.binList)) for s in g] for g in r] for r in (a, b)]
    assert results[True] == results[False]


@pytest.mark.parametrize("name", ["n160", "n300_edges", "n400_default", "n500_sparse"])
def test_golden_maps_both_ways(hic, monkeypatch, tmp_path, name):
    """The golden pipelines' Part 2 with the batched calls and without: the reference's files both times, the same
    printed lines."""
    from hic_genome_assembler_amd import scaffoldToChromosomes as p1, orderGenome as p2
    spec = gc.load_case(name)[0]
    paths = gc.write_case_files(name, str(tmp_path))
    f = lambda k: os.path.join(str(tmp_path), k)  # noqa: E731
    with contextlib.redirect_stdout(io.StringIO()):
        p1.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                       paths["hicProScaffSizeFile"], f("dendrogramOrder.txt"), f("a.png"), f("b.png"),
                       f("binGroups.txt"), f("assessment.txt"), f("chromosomeGroups.txt"),
                       True, False, spec["min_size"], 0.0, 20, spec["psig"], 5, .2, 100000)
    lines = {}
    for flag in (True, False):
        _flags(monkeypatch, p2, flag, flag)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            p2.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                           f("chromosomeGroups.txt"), f("chromosomeOrders.txt"), str(tmp_path), "synthetic", f("g.png"),
                           "synthetic genome", f("plotOrder.txt"), spec["n_scaffolds"], spec["scan_scaffolds"], 100000)
        for fn in P2_FILES:
            with open(f(fn)) as fh:
                assert fh.read() == gc.golden_text(name, fn), (fn, flag)
        lines[flag] = sorted(ln for ln in _drop_clock(buf.getvalue()) if not ln.startswith("Total run-time"))
    assert lines[True] == lines[False]


@pytest.mark.parametrize("n", [3000, 6000])
def test_synthetic_maps_both_ways(hic, monkeypatch, tmp_path, n):
    """bench.py's kind of map at 3,000 and 6,000 bins, its true chromosomes as the groups: batched start + arranged scan
    against the per-chromosome start + scanOrdering, and each of the two switches on its own."""
    import torch
    from hic_genome_assembler_amd import orderGenome as p2, synth
    lay = synth.make_layout(n, seed=2)
    ct = synth.dense_contacts_torch(lay, torch.device("cuda", 0), seed=2, sinkhorn_iters=12)
    torch.cuda.synchronize()
    chromList = [[] for _ in range(int(lay.chrom_of_bin.max()) + 1)]
    for b in range(n):
        chromList[int(lay.chrom_of_bin[b])].append([b + 1, lay.scaffold_names[lay.scaffold_of_bin[b]]])
    chromList = [c for c in chromList if c]
    runs = []
    for k, (start_all, scan_arranged) in enumerate([(True, True), (False, False), (True, False), (False, True)]):
        _flags(monkeypatch, p2, start_all, scan_arranged)
        runs.append(_order_genome(hic, p2, None, chromList, 6, 5, str(tmp_path / str(k)), device_ptr=(ct.data_ptr(), n, ct)))
    assert not isinstance(runs[0][0], tuple)
    assert sum(len(g) > 6 for g in runs[0][0]) >= 3              # chromosomes that were scanned
    for other in runs[1:]:
        _same_runs(runs[0], other)


def test_start_states_equal_per_chromosome_states(hic, monkeypatch):
    """_startAll against _startChromosome on contexts of their own: the brute-force order and orientations, the
    scaffolds left to insert, every Scaffold's bins, the layout and what was printed, chromosome by chromosome."""
    from hic_genome_assembler_amd import orderGenome as p2
    chromList, n, contacts = _mixed()
    todo = sorted(range(len(chromList)), key=lambda i: -len(chromList[i]))
    bins = _bin_objects(n)
    out = {}
    for batched in (True, False):
        with hic.Context(0) as ctx:
            ctx.set_contacts(contacts)
            lanes, _p, _j = _jobs(p2, ctx, chromList, n, 6, todo)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                if batched:
                    states = p2._startAll(todo, chromList, lanes, bins, 6, 5)
                else:
                    states = {}
                    for i in todo:
                        print("#####################\n#####################")
                        print("Working on Chr_" + str(i + 1) + "...")
                        states[i] = p2._startChromosome(chromList[i], lanes[i], bins, 6, 5)
            view = lambda ss: [(s.name, s.orientation, list(s.binList)) for s in ss]  # noqa: E731
            out[batched] = ({i: (view(st["ordered"]), view(st["rest"]), view(st["dict"].values()), len(st["orderDict"]), dict(st["orderDict"]),
                                 st["nScaffolds"], st["scanScaffolds"], lanes[i].chrom.sid, lanes[i].chrom.start,
                                 lanes[i].chrom.length, lanes[i].chrom.names, lanes[i].chrom._tables_k)
                             for i, st in states.items()}, buf.getvalue())
    assert out[True][0] == out[False][0]
    assert out[True][1] == out[False][1]
