"""Part 2's batched start phase on the CPU: a context without hicmi_p2_start_all (tests/fake_context.py) takes the
per-chromosome path and gives today's files, and the flat arrays built for the batched call are what ChromosomeLayout
builds chromosome by chromosome."""
import os
import types

import numpy as np
import pytest

import golden_cases as gc
from fake_context import OracleContext

CASES = ["n160", "n300_edges", "n400_default"]


class LaneContext(OracleContext):
    """The double with worker contexts, so that orderGenome takes its lock-step branch: no p2_start_all, no fused
    decision steps - every chromosome's insertion job is None and the start phase must fall back."""

    def workers(self, count):
        out = []
        for _ in range(count):
            w = LaneContext()
            w.set_contacts(self.mat)
            out.append(w)
        return out

    @staticmethod
    def p2_insert_all_multi(jobs):
        assert jobs == []
        return []


@pytest.fixture()
def fake_gpu(monkeypatch):
    from hic_genome_assembler_amd import _lib
    monkeypatch.setattr(_lib, "Context", LaneContext)
    monkeypatch.setattr(_lib, "hypergeom_sf", lambda x, M, n, N: float(__import__("hic_oracle").hyper_geom(x, M, n, N)))
    return _lib


@pytest.mark.parametrize("name", CASES)
def test_context_without_the_call_takes_the_per_chromosome_start(fake_gpu, monkeypatch, name, tmp_path):
    from hic_genome_assembler_amd import orderGenome as p2, scaffoldToChromosomes as p1
    assert p2.START_ALL and not p2._start_all_applies(LaneContext())
    started, batched = [], []
    real = p2._startChromosome
    monkeypatch.setattr(p2, "_startChromosome", lambda *a, **k: (started.append(1), real(*a, **k))[1])
    monkeypatch.setattr(p2, "_startAll", lambda *a, **k: batched.append(1))
    spec = gc.load_case(name)[0]
    paths = gc.write_case_files(name, str(tmp_path))
    f = lambda k: os.path.join(str(tmp_path), k)  # noqa: E731
    p1.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                   paths["hicProScaffSizeFile"], f("dendrogramOrder.txt"), f("a.png"), f("b.png"),
                   f("binGroups.txt"), f("assessment.txt"), f("chromosomeGroups.txt"),
                   True, False, spec["min_size"], 0.0, 20, spec["psig"], 5, .2, 100000)
    p2.runPipeline(paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                   f("chromosomeGroups.txt"), f("chromosomeOrders.txt"), str(tmp_path), "synthetic", f("g.png"),
                   "synthetic genome", f("plotOrder.txt"), spec["n_scaffolds"], spec["scan_scaffolds"], 100000)
    n_chrom = len(p2.readChromsFromFile(f("chromosomeGroups.txt")))
    assert len(started) == n_chrom and not batched
    for fn in gc.OUTPUT_FILES:
        with open(f(fn)) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn


def test_switches_that_keep_the_per_chromosome_start(monkeypatch):
    from hic_genome_assembler_amd import orderGenome as p2
    ctx = types.SimpleNamespace(p2_start_all=lambda jobs, tables: [])
    assert p2._start_all_applies(ctx)
    for name, value in (("START_ALL", False), ("START_THREADS", 2), ("SCORE_HOOK", lambda fast: None)):
        with monkeypatch.context() as m:
            m.setattr(p2, name, value)
            assert not p2._start_all_applies(ctx)
    assert p2._start_all_applies(ctx)


class RecordingContext:
    def __init__(self):
        self.calls = []

    def p2_select(self, sel):
        self.calls.append(("select", [int(v) for v in sel]))

    def p2_layout(self, start, length):
        self.calls.append(("layout", [int(v) for v in start], [int(v) for v in length]))


@pytest.mark.parametrize("n_scaffolds", [1, 3, 6, 8])
def test_flat_arrays_equal_what_the_layout_builds(n_scaffolds):
    """_startJobs' tuples against ChromosomeLayout's own p2_select / p2_layout arguments, chromosome by chromosome; the
    layout built for the batched call issues nothing itself, and the scaffolds of the brute force are the first
    min(nScaffolds, S) of the size-sorted list."""
    import contextlib
    import io
    from hic_genome_assembler_amd import orderGenome as p2
    rng = np.random.default_rng(4)
    ids = rng.permutation(400) + 1                               # bin IDs in no particular row order
    bins = [types.SimpleNamespace(ID=int(v)) for v in ids]
    chromList, used = [], 0
    for c, n_scaf in enumerate([1, 2, 5, 9, 17]):
        rows = []
        for s in range(n_scaf):
            ln = int(rng.integers(1, 9))
            rows += [[int(v), "c%d_s%d" % (c, s)] for v in sorted(ids[used:used + ln], reverse=bool(s % 2))]
            used += ln
        rows = [rows[i] for i in rng.permutation(len(rows))]     # the group file lists bins, not scaffolds, in order
        chromList.append(rows)
    todo = [3, 0, 4, 1, 2]
    lanes = {i: p2.GenomeMatrix(RecordingContext()) for i in todo}
    for m in lanes.values():
        m.bin_index(bins)
    prepared, jobs = p2._startJobs(todo, chromList, lanes, bins, n_scaffolds)
    assert [j[0] for j in jobs] == [lanes[i].ctx for i in todo]
    for i, (ctx, sel, start, length, first) in zip(todo, jobs):
        assert ctx.calls == []                                   # nothing issued by the batched layout
        ref = p2.GenomeMatrix(RecordingContext())
        ref.bin_index(bins)
        with contextlib.redirect_stdout(io.StringIO()):
            scaffs, _d = p2.initiateBinsAndScaffolds(chromList[i])
        layout = p2.ChromosomeLayout(ref, scaffs, bins)
        assert ref.ctx.calls == [("select", [int(v) for v in sel]), ("layout", list(start), list(length))]
        got_layout, ordered, rest, scaff_dict = prepared[i]
        assert (got_layout.sid, got_layout.start, got_layout.length, got_layout.names, got_layout.n) == \
            (layout.sid, layout.start, layout.length, layout.names, layout.n)
        k = min(n_scaffolds, len(scaffs))
        assert list(first) == list(range(k)) and [s.name for s in ordered] == [s.name for s in scaffs[:k]]
        assert [s.name for s in rest] == [s.name for s in scaffs[k:]]
        assert sorted(scaff_dict) == sorted(s.name for s in scaffs)
        where = {b.ID: r for r, b in enumerate(bins)}
        assert [int(v) for v in sel] == [where[b] for s in scaffs for b in sorted(s.binList)]
