"""What the context-reuse tests run: the stage families with their three cases (FAMILIES), the calls that put another
matrix or other sums under a context (REPLACERS), the calls that answer from state derived from the matrix (DEPENDENTS),
and the two tables that tests/test_reuse_cpu.py holds against the source: every device and pinned buffer of hicmi_ctx with
the families whose second or third case regrows it (BUFFERS), and every function of the driver that replaces the matrix
or the sums with the replacer that reaches it (REPLACER_SITES).

A family is a function run(ctx, case) -> {name: array}: every array and scalar the family's entry points hand back.  The
entry "sizes" lists what the family allocates by (bins, scaffolds, cells, records, T): the tests assert from it that a
later case needs more than an earlier one.  Inputs come from synth and from the helpers of the families' own test files
and *_reference.py modules."""
import contextlib
import functools
import os

import numpy as np

import liftmap_reference as lref
import span_reference as sref
import split_reference as splitref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (192, 320, 192)                 # the third map is another map than the first: nothing stale may answer for it
ENV = ("HICMI_NO_PRESORT", "HICMI_SORT_RADIX", "HICMI_SORT_LDS", "HICMI_PRESORT_TIES", "HICMI_HOST_SCANS", "HICMI_REBIN_PLAIN",
       "HICMI_ICE_INPLACE", "HICMI_P2_DEVICE_DECIDE", "HICMI_PAIRS_PLAIN", "HICMI_PAIRS_FIRST_PAIRS", "HICMI_ENDS_PLAIN",
       "HICMI_ANCHOR_PLAIN", "HICMI_SPANS_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS", "HICMI_BUILDMAP_PLAIN", "HICMI_LIFTMAP_PLAIN",
       "HICMI_SPLIT_PLAIN", "HICMI_SEATS_PLAIN", "HICMI_LINKS_PLAIN")


def default_forms(monkeypatch):
    """Every family in its default kernel form; the pre-sort buffers are built at these sizes."""
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("HICMI_PRESORT_FROM", "64")


def _i(*values):
    return np.array(values, np.int64)


# ---- matrix cases ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix_cases():
    from hic_genome_assembler_amd import synth
    out = []
    for k, n in enumerate(SIZES):
        layout = synth.make_layout(n, seed=11 + k)
        c = synth.dense_contacts(layout, seed=11 + k)
        c.setflags(write=False)
        out.append((layout, c))
    return tuple(out)


def selection(layout):
    """Part 2 on the bins of the planted chromosomes 0 .. 3 (half the map): the selection and its scaffold ranges."""
    sel = np.flatnonzero(layout.chrom_of_bin < 4).astype(np.int32)
    scaf = layout.scaffold_of_bin[sel]
    starts = np.flatnonzero(np.r_[True, scaf[1:] != scaf[:-1]]).astype(np.int32)
    lens = np.diff(np.r_[starts, len(sel)]).astype(np.int32)
    return sel, starts, lens


@functools.lru_cache(maxsize=None)
def window_tables(k):
    from hic_genome_assembler_amd import orderGenome as p2
    orders, orients = p2._enumeration(k)
    return (np.asarray(orders, np.int8), np.asarray([[1 if sg == "-" else 0 for sg in r] for r in orients], np.uint8))


def _cut_lists(got, prefix, results):
    for j, (a, b) in enumerate(results):
        got["%s%d" % (prefix, j)] = np.array(a, np.int64)
        got["%s%d_log" % (prefix, j)] = np.array(b, np.int64).reshape(-1, 2) if isinstance(b, list) else _i(b)


def run_part1(ctx, case):
    """row_sums, upgma, rank_matrix, a similarity row, the two cut scans and their lock-step forms with 3 sets."""
    _layout, c = case
    n = len(c)
    got = {"sizes": _i(n)}
    ctx.set_contacts(c)
    got["np_sum"], got["seq_sum"] = ctx.row_sums()
    got["leaves"], got["Z"] = ctx.upgma()
    got["raw_merges"] = ctx.raw_merges()
    ctx.rank_matrix(got["leaves"])
    got["presort"] = np.array(ctx.presort_state())
    got["rank"], got["rank_inverse"] = ctx.rank_rows(), ctx.rank_rows(inverse=True)
    got["similarity"] = ctx.similarity_row(n // 3)
    got["cut_sig"], got["cut_x"] = ctx.cut_scan(3, n - 3, .05, want_x=True)
    got["filter_sig"], got["filter_x"] = ctx.filter_scan(3, n // 2, n // 4, n - 3, .01, want_x=True)
    stop = int(n - n * .05)
    cuts, m_log = ctx.first_pass_cuts(5, stop, .05)
    kept, warned = ctx.filter_cuts(cuts, .05)
    got["cuts"], got["m_log"] = np.array(cuts), np.array(m_log).reshape(-1, 2)
    got["kept"], got["warned"] = np.array(kept), np.array([warned])
    multi = ctx.first_pass_cuts_multi([(5, stop), (9, stop), (14, n - 1)], .05)
    _cut_lists(got, "first_multi", multi)
    _cut_lists(got, "filter_multi", ctx.filter_cuts_multi([multi[0][0], multi[1][0], multi[2][0][::2]], [.05, .01, .05]))
    # the same map in whole counts: rows that hold equal similarities, whose order the pre-sort leaves to a second pass
    # (d_row_list is reserved on that path alone)
    ctx.set_contacts(np.floor(c))
    got["tied_leaves"], got["tied_Z"] = ctx.upgma()
    ctx.rank_matrix(got["tied_leaves"])
    got["tied_presort"] = np.array(ctx.presort_state())
    got["tied_rank"] = ctx.rank_rows()
    return got


def _arranged(ctx, case):
    layout, c = case
    ctx.set_contacts(c)
    sel, starts, lens = selection(layout)
    ctx.p2_select(sel)
    ctx.p2_layout(starts, lens)
    return sel, starts, lens


def run_p2_tables(ctx, case):
    """Placement, break and inversion support through the _multi forms with one job."""
    sel, starts, lens = _arranged(ctx, case)
    ids = np.arange(len(starts), dtype=np.int32)
    rev = (ids % 3 == 1).astype(np.uint8)
    ctx.p2_set_arrangement(ids, rev)
    total = ctx.p2_arrangement_total()
    got = {"sizes": _i(len(case[1]), len(sel), len(starts), int((lens - 1).sum())), "total": np.array([total])}
    (got["support"], got["support_best"]), = type(ctx).p2_support_multi([(ctx, ids, rev, total)])
    (got["breaks"], got["breaks_best"]), = type(ctx).p2_breaks_multi([(ctx, ids, rev, lens, total)])
    (got["inversions"], got["inversions_best"]), = type(ctx).p2_inversions_multi([(ctx, ids, rev, total)])
    return got


def _short_lists(got, prefix, lists):
    for w, entry in enumerate(lists):
        got["%s%d_overflow" % (prefix, w)] = _i(entry is None)
        if entry is not None:
            got["%s%d_index" % (prefix, w)], got["%s%d_fast" % (prefix, w)] = entry


def run_p2_search(ctx, case):
    """The scores, the insertion scores, windows of 3 (tables, deltas, short lists, one decision), a short list of windows
    of 7 (the device's near-top lists), the insertion loop and the scan from its arrangement."""
    sel, starts, lens = _arranged(ctx, case)
    S = len(starts)
    rng = np.random.default_rng(S)
    perms = np.stack([rng.permutation(len(sel)) for _ in range(5)]).astype(np.int32)
    total = ctx.p2_total()
    got = {"sizes": _i(len(case[1]), len(sel), S), "p2_total": np.array([total])}
    got["score"], got["score_exact"] = ctx.p2_score(perms, total), ctx.p2_score_exact(perms, total)
    placed = np.arange(S - 3, dtype=np.int32)
    rev = (placed % 3 == 1).astype(np.uint8)
    ctx.p2_set_arrangement(placed, rev)
    atotal = ctx.p2_arrangement_total()
    cur = ctx.p2_arrangement_score(atotal)
    got["arrangement"] = np.array([atotal, cur])
    got["insertions"] = ctx.p2_score_insertions(S - 1, atotal)
    ctx.p2_window_tables(*window_tables(7))
    _short_lists(got, "near7_", ctx.p2_window_shortlist(0, 1, 7, atotal, 0.0, cur))
    ctx.p2_window_tables(*window_tables(3))
    got["window"] = ctx.p2_score_window(1, 3)
    _short_lists(got, "near3_", ctx.p2_window_shortlist(0, 3, 3, atotal, 0.0, cur))
    got["decide"] = np.array(ctx.p2_decide_window(1, 3, atotal, 0.0, cur), np.float64)
    ids, rv, best = ctx.p2_insert_all(placed, rev, np.arange(S - 3, S, dtype=np.int32))
    got["inserted_ids"], got["inserted_rev"], got["inserted_best"] = ids.copy(), rv.copy(), np.array([best])
    ids, rv, best, rounds, stotal = ctx.p2_scan_arranged(ids, rv, 3, *window_tables(3), best)
    got["scanned_ids"], got["scanned_rev"], got["scanned"] = ids, rv, np.array([best, rounds, stotal])
    return got


def run_hmm(ctx, case):
    """The observation matrix of the leaf order in slot 0 and a narrower, shorter one in slot 1; the single-problem calls
    on slot 0 and the _multi calls over both."""
    _layout, c = case
    n = len(c)
    ctx.set_contacts(c)
    ctx.row_sums()
    leaves, _z = ctx.upgma(want_linkage=False)
    cut, prev = n // 8, n // 2
    T, D = ctx.hmm_load_obs(leaves, cut, prev)
    got = {"sizes": _i(n, T, D), "obs": ctx.hmm_get_obs()}
    got["mean"], got["m2"] = ctx.hmm_col_stats()
    got["dist2"] = ctx.hmm_dist2([1, T - 2])
    centers, got["labels"], inertia, iters = ctx.hmm_kmeans(got["obs"][[1, T - 2]], max_iter=20)
    got["centers"], got["kmeans"] = centers, np.array([inertia, iters])
    covars = np.tile(np.maximum(got["m2"] / T, 1e-3), (2, 1))
    start, trans = np.array([.5, .5]), np.array([[.9, .1], [.2, .8]])
    got["fit_means"], got["fit_covars"], got["fit_trans"], got["fit_logprob"] = ctx.hmm_fit(start, centers, covars, trans, n_iter=4)
    got["states"] = ctx.hmm_decode(start, got["fit_means"], got["fit_covars"], got["fit_trans"])
    T1, D1 = ctx.hmm_load_obs_slot(1, leaves, n // 4, n // 3)
    got["sizes"] = _i(n, T, D, T1, D1)
    problems = [(0, D, (0, T - 1)), (1, D1, (2,)), (0, D // 2, (3, 5))]
    for j, d in enumerate(ctx.hmm_dist2_multi(problems)):
        got["dist2_multi%d" % j] = d
    kproblems = [(0, D, (1, T - 2), 20, 0.0), (1, D1, (0, T1 - 1), 20, 0.0), (0, D // 2, (2, T // 2), 5, 0.0)]
    for j, (cen, inertia, iters) in enumerate(ctx.hmm_kmeans_multi(kproblems)):
        got["kmeans_multi%d" % j], got["kmeans_multi%d_end" % j] = cen, np.array([inertia, iters])
    return got


def run_louvain(ctx, case):
    """The graph of every second row, level 0 from three fixed generator states, an induced graph and the modularities."""
    _layout, c = case
    n = len(c)
    ctx.set_contacts(c)
    ctx.row_sums()
    rows = np.arange(0, n, 2, dtype=np.int32)
    m = ctx.louvain_graph(rows)
    got = {"sizes": _i(n, m)}
    got["A"], got["gdegrees"], tw = ctx.louvain_get_graph()
    got["total_weight"] = np.array([tw])
    states = [np.random.Generator(np.random.PCG64(seed)).bit_generator.state for seed in (1, 2, 3)]
    n2c, after, got["info"], got["degrees"], got["internals"] = ctx.louvain_level0(states)
    got["node2com"] = n2c
    got["states_after"] = np.array([[s["state"]["state"] & (2 ** 64 - 1), s["state"]["state"] >> 64, s["has_uint32"], s["uinteger"]]
                                    for s in after], np.uint64)
    part = (np.arange(m) % 5).astype(np.int32)
    got["induced"] = ctx.louvain_induced(part, 5)
    got["modularity"] = ctx.louvain_modularity(np.vstack([n2c, part[None, :]]))
    return got


def run_group_junction(ctx, case):
    """Group sums on the planted chromosomes (a tenth of the bins in no group) and junction sums over views of both
    directions of a permuted bin list."""
    layout, c = case
    n = len(c)
    ctx.set_contacts(c)
    grp = layout.chrom_of_bin.astype(np.int32).copy()
    grp[::10] = -1
    scaf = layout.scaffold_of_bin.astype(np.int32)
    G, S = int(layout.chrom_of_bin.max()) + 1, int(scaf.max()) + 1
    got = {"sizes": _i(n, S)}
    got["group_bins"], got["group_scaffolds"] = ctx.group_sums(grp, scaf, G, S)
    bins = np.random.default_rng(n).permutation(n).astype(np.int32)
    rec = [(0, 1, n // 3, n // 3, 1, n // 4), (n - 1, -1, n // 2, 0, 1, 70), (5, 1, 1, 9, -1, 1), (n // 2, -1, 65, n // 2 + 1, 1, n // 2 - 2)]
    rec += [(k, 1, 3, k + 3, 1, 4) for k in range(0, n - 8, 7)]
    got["junction_sums"] = ctx.junction_sums(bins, rec)
    got["sizes"] = _i(n, S, len(rec))
    return got


def run_plot(ctx, case):
    """Percentiles and block means of the three kinds of matrix, whole and on a permuted subset."""
    _layout, c = case
    n = len(c)
    ctx.set_contacts(c)
    ctx.row_sums()
    order = np.random.default_rng(n + 1).permutation(n)[:n - n // 5].astype(np.int32)
    got = {"sizes": _i(n, len(order), n // 5)}
    for kind in (0, 1, 2):
        got["percentiles%d" % kind] = ctx.plot_percentiles(kind, order, [1.0, 50.0, 99.5])
        got["percentiles%d_whole" % kind] = ctx.plot_percentiles(kind, None, [0.0, 37.5, 100.0])
        got["image%d" % kind] = ctx.plot_downsample(kind, order, n // 5)
    return got


def run_ice(ctx, case):
    """Masked rows, the balancing on its default path, and the matrix it leaves."""
    _layout, c = case
    n = len(c)
    ctx.set_contacts(c)
    mask = (np.arange(n) % 17 == 5).astype(np.uint8)
    ctx.ice_mask_rows(mask)
    got = {"sizes": _i(n), "masked": ctx.contacts_host()}
    bias, iters, delta = ctx.ice_balance(mask=(np.arange(n) % 23 == 7).astype(np.uint8), max_iter=12, eps=0.0)
    got["bias"], got["ice_end"] = bias, np.array([iters, delta])
    got["balanced"] = ctx.contacts_host()
    got["np_sum"], got["seq_sum"] = ctx.row_sums()
    return got


def run_rebin(ctx, case):
    """The map at 2 fine bins per coarse bin, and that one at 3 (the last coarse bin narrower)."""
    _layout, c = case
    n = len(c)
    ctx.set_contacts(c)
    got = {"sizes": _i(n)}
    for by in (2, 3):
        m = ctx.n
        ctx.rebin(np.r_[np.arange(0, m, by), m].astype(np.int32))
        got["by%d" % by] = ctx.contacts_host()
        got["by%d_np_sum" % by], got["by%d_seq_sum" % by] = ctx.row_sums()
    return got


MATRIX_FAMILIES = {"part1": run_part1, "p2_tables": run_p2_tables, "p2_search": run_p2_search, "hmm": run_hmm,
                   "louvain": run_louvain, "group_junction": run_group_junction, "plot": run_plot, "ice": run_ice,
                   "rebin": run_rebin}


# ---- pair cases -----------------------------------------------------------------------------------------------------------
WINDOW, REACH, STEP, FLANK = 500, 2, 250, 2
RESOLUTIONS = (1500, 4000)


class PairCase:
    """Scaffold sizes, chromosomes as lists of (scaffold, "+" / "-"), and pairs (scaffold a, position a, scaffold b,
    position b); the lift tables with the unplaced scaffolds as sequences of their own (``tables``) and dropped
    (``dropped``)."""

    def __init__(self, sizes, chroms, pairs):
        self.sizes, self.chroms, self.pairs = np.asarray(sizes, np.int64), chroms, pairs
        self.tables = lref.layout(chroms, self.sizes, 100)
        self.dropped = lref.layout(chroms, self.sizes, 100, drop_unplaced=True)
        for a in (self.sizes,) + tuple(pairs) + tuple(self.tables) + tuple(self.dropped):
            a.setflags(write=False)

    def chunks(self, k):
        edges = [len(self.pairs[0]) * j // k for j in range(k + 1)]
        return [tuple(a[lo:hi] for a in self.pairs) for lo, hi in zip(edges[:-1], edges[1:])]

    def rank_target(self):
        """Rank mode of the anchoring: the dropped scaffolds in turn against every chromosome and against nothing."""
        target = np.full(len(self.sizes), -1, np.int32)
        for k, s in enumerate(np.flatnonzero(self.dropped[0] < 0).tolist()):
            target[s] = k % (len(self.chroms) + 1) - 1
        return target

    def measures(self):
        return [len(self.sizes), len(self.pairs[0]), int(self.sizes.sum())]


def _drawn_case(n_scaf, n_placed, n_chrom, n_pairs, seed):
    """Scaffolds of 600 .. 12,000 bases (one of one base), ``n_placed`` of them in ``n_chrom`` chromosomes, and pairs: six
    in ten between two scaffolds of one chromosome, one in ten on one scaffold, the rest anywhere."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(600, 12001, n_scaf).astype(np.int64)
    sizes[n_scaf // 2] = 1
    placed = rng.permutation(n_scaf)[:n_placed]
    chroms = [[(int(s), "+-"[int(rng.integers(0, 2))]) for s in part] for part in np.array_split(placed, n_chrom)]
    member = [np.array([s for s, _o in ch]) for ch in chroms]
    kind = rng.random(n_pairs)
    ch = rng.integers(0, n_chrom, n_pairs)
    sa = np.where(kind < .6, [rng.choice(member[q]) for q in ch], rng.integers(0, n_scaf, n_pairs))
    sb = np.where(kind < .6, [rng.choice(member[q]) for q in ch], rng.integers(0, n_scaf, n_pairs))
    sb = np.where((kind >= .6) & (kind < .7), sa, sb)
    pa = 1 + np.floor(rng.random(n_pairs) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n_pairs) * sizes[sb]).astype(np.int64)
    return PairCase(sizes, chroms, (sa.astype(np.int32), pa, sb.astype(np.int32), pb))


@functools.lru_cache(maxsize=None)
def pair_cases():
    """The 40 odd scaffolds, chromosomes and 5,000 pairs of test_gpu_ends; 8 scaffolds with 300 pairs; 52 other scaffolds
    with 12,000 pairs.  The second is smaller than the first in every measure and the third larger than both, so every
    table, grid and store meets a smaller problem in memory it keeps and then regrows."""
    import test_gpu_ends as ge
    _names, sizes = ge._scaffolds()
    return (PairCase(sizes.copy(), ge.CHROMS, tuple(a.copy() for a in ge._pool())), _drawn_case(8, 6, 2, 300, 21),
            _drawn_case(52, 28, 4, 12000, 22))


def _map_out(got, ctx, key):
    got[key] = ctx.contacts_host()
    got[key + "_np_sum"], got[key + "_seq_sum"] = ctx.row_sums()


def run_buildmap(ctx, case):
    got = {"sizes": _i(*case.measures())}
    for res in RESOLUTIONS:
        ctx.map_begin(case.sizes, res)
        for part in case.chunks(2):
            ctx.map_add_pairs(*part)
        got["pairs%d" % res] = _i(ctx.map_finish())
        _map_out(got, ctx, "map%d" % res)
    return got


def run_liftmap(ctx, case):
    got = {"sizes": _i(*case.measures())}
    for res in RESOLUTIONS:
        ctx.map_begin_lifted(case.sizes, *case.tables, res)
        for part in case.chunks(2):
            ctx.map_add_pairs(*part)
        got["pairs%d" % res] = _i(ctx.map_finish())
        _map_out(got, ctx, "map%d" % res)
    stats = None
    for part in case.chunks(2):
        stats = ctx.pair_stats(*part, case.sizes, *case.tables, into=stats)
    got["decay"], got["seq_cis"], got["seq_trans"], got["unlifted"] = stats
    return got


def span_records(case):
    """The records of a report, and every sequence as one record (as tests/test_gpu_spans.py asks for them)."""
    scaf, junc = sref.report_records(case.sizes, case.tables, STEP)
    _cell_first, seq_first, _n = sref.number_cells(case.sizes, case.tables, STEP)
    whole = [(int(a), int(b) - 1, int(a), int(b)) for a, b in zip(seq_first[:-1], seq_first[1:]) if b > a]
    return np.asarray(list(scaf.values()) + list(junc.values()) + whole, np.int64).reshape(-1, 4)


def run_spans(ctx, case):
    recs = span_records(case)
    got = {"cell_first": ctx.span_begin(case.sizes, *case.tables, STEP, 0)}
    for part in case.chunks(2):
        ctx.span_add_pairs(*part)
    got["picks"], got["counters"], got["depth"] = ctx.span_finish(FLANK, recs)
    got["sizes"] = _i(*case.measures(), len(got["depth"]), len(recs))
    return got


def run_ends(ctx, case):
    got = {"rank": ctx.ends_begin(case.sizes, *case.tables, WINDOW, REACH)}
    for part in case.chunks(2):
        ctx.ends_add_pairs(*part)
    got["table"], got["counters"] = ctx.ends_finish()
    got["sizes"] = _i(*case.measures(), got["table"].size)
    return got


def run_anchor(ctx, case):
    got, cells = {}, []
    for mode, target in (("sequence", None), ("rank", case.rank_target())):
        got[mode + "_first"] = ctx.anchor_begin(case.sizes, *case.dropped, target, WINDOW)
        for part in case.chunks(2):
            ctx.anchor_add_pairs(*part)
        got[mode + "_table"], got[mode + "_counters"] = ctx.anchor_finish()
        cells.append(len(got[mode + "_table"]))
    got["sizes"] = _i(*case.measures(), *cells)
    return got


def split_pieces(case):
    """Every fourth scaffold of two bases or more cut in the middle, the longest one into five pieces."""
    cuts = {int(s): [int(case.sizes[s]) // 2] for s in np.flatnonzero(case.sizes > 1)[::4].tolist()}
    longest = int(np.argmax(case.sizes))
    cuts[longest] = [int(case.sizes[longest]) * j // 5 for j in range(1, 5)]
    first, start, _size, _parent = splitref.make_pieces(case.sizes, cuts)
    return first, start


def run_split(ctx, case):
    first, start = split_pieces(case)
    got = {"sizes": _i(*case.measures(), len(start))}
    counters = None
    for j, part in enumerate(case.chunks(2)):
        ka, xa, kb, xb, counters = ctx.split_pairs(*part, case.sizes, first, start, into=counters)
        got.update({"piece_a%d" % j: ka, "pos_a%d" % j: xa, "piece_b%d" % j: kb, "pos_b%d" % j: xb})
    got["counters"] = counters
    return got


def load_store(ctx, case):
    ctx.pairs_begin(case.sizes)
    for part in case.chunks(3):
        ctx.pairs_add(*part)


def read_store(ctx, case):
    """The store in its default (stable) form: the kept pairs in the order they were added."""
    got = {"sizes": _i(*case.measures())}
    n_kept, n_intra, got["intra"] = ctx.pairs_info()
    got["info"] = _i(n_kept, n_intra)
    got["scaf_a"], got["pos_a"], got["scaf_b"], got["pos_b"] = ctx.pairs_fetch()
    return got


def run_pairs_store(ctx, case):
    load_store(ctx, case)
    try:
        return read_store(ctx, case)
    finally:
        ctx.pairs_drop()


def read_resident(ctx, case):
    """Every stage that reads the resident store.  The rows of both link graphs come back sorted by (lo, hi), whatever
    slots the race for the table gave them."""
    got = {"sizes": _i(*case.measures())}
    got["ends_rank"], got["ends_table"], got["ends_counters"] = ctx.ends_resident(case.sizes, *case.tables, WINDOW, REACH)
    got["anchor_first"], got["anchor_table"], got["anchor_counters"] = ctx.anchor_resident(case.sizes, *case.dropped,
                                                                                          case.rank_target(), WINDOW)
    got["seats_first"], got["seats_table"], got["seats_counters"] = ctx.seats_resident(case.sizes, *case.tables, WINDOW)
    got["links_lo"], got["links_hi"], got["links_counts"], got["links_counters"] = ctx.links_resident(case.sizes, WINDOW)
    got["lifted_lo"], got["lifted_hi"], got["lifted_counts"], got["lifted_counters"] = ctx.links_lifted(case.sizes, *case.tables,
                                                                                                    WINDOW)
    got["sizes"] = _i(*case.measures(), got["ends_table"].size, len(got["anchor_table"]), len(got["seats_table"]),
                      len(got["links_lo"]))
    return got


def run_resident(ctx, case):
    load_store(ctx, case)
    try:
        return read_resident(ctx, case)
    finally:
        ctx.pairs_drop()


PAIR_FAMILIES = {"buildmap": run_buildmap, "liftmap": run_liftmap, "spans": run_spans, "ends": run_ends, "anchor": run_anchor,
                 "split": run_split, "pairs_store": run_pairs_store, "resident": run_resident}
FAMILIES = dict(MATRIX_FAMILIES, **PAIR_FAMILIES)
# further kernel forms of a family, where its own test file parametrises them: {family: {form: environment}}
PLAIN_FORMS = {"rebin": {"HICMI_REBIN_PLAIN": "1"}, "buildmap": {"HICMI_BUILDMAP_PLAIN": "1"},
               "liftmap": {"HICMI_LIFTMAP_PLAIN": "1"}, "spans": {"HICMI_SPANS_PLAIN": "1"}, "ends": {"HICMI_ENDS_PLAIN": "1"},
               "anchor": {"HICMI_ANCHOR_PLAIN": "1"}, "split": {"HICMI_SPLIT_PLAIN": "1"}, "pairs_store": {"HICMI_PAIRS_PLAIN": "1"},
               "resident": {"HICMI_SEATS_PLAIN": "1", "HICMI_LINKS_PLAIN": "1", "HICMI_ENDS_PLAIN": "1", "HICMI_ANCHOR_PLAIN": "1"}}


def cases_of(family):
    return matrix_cases() if family in MATRIX_FAMILIES else pair_cases()


def canonical(family, form, got):
    """``got`` in the form two runs can be compared in.  One output depends on a race by design: a pair store built with
    HICMI_PAIRS_PLAIN=1 keeps its pairs in the order the workgroups of a chunk won their places, so its
    rows are compared sorted, as tests/test_gpu_pairs.py compares them."""
    if family == "pairs_store" and form == "plain":
        import pairs_reference as pref
        rows = pref.sorted_rows((got["scaf_a"], got["pos_a"], got["scaf_b"], got["pos_b"]))
        got = {k: v for k, v in got.items() if k not in ("scaf_a", "pos_a", "scaf_b", "pos_b")}
        got["rows_sorted"] = np.asarray(rows)
    return got


# ---- what a matrix change invalidates ---------------------------------------------------------------------------------------
# The chain of state a context derives from its matrix, in the order it is built.  Its inputs depend on nothing but
# "the map has at least 96 bins", so that the same calls are valid before and after every replacer: a stale context
# then has nothing to refuse them for but the missing step.
SEL = np.arange(8, 80, dtype=np.int32)
LENS = np.array([9, 7, 11, 5, 8, 6, 10, 4, 12], np.int32)
STARTS = (np.cumsum(LENS) - LENS).astype(np.int32)
IDS = np.arange(7, dtype=np.int32)
REV = np.array([0, 1, 0, 0, 1, 1, 0], np.uint8)
NEW_IDS = np.array([7, 8], np.int32)
TOTAL = 1000.0                          # the scores divide by it and nothing else
PERMS = np.stack([np.random.default_rng(5).permutation(len(SEL)) for _ in range(4)]).astype(np.int32)
CUTS = [24, 48, 72]

CHAIN = ("upgma", "rank_matrix", "p2_select", "p2_layout", "p2_set_arrangement")


def build_chain(ctx, leaves=None):
    """Every piece of derived state, rebuilt from the matrix the context holds; the window tables of 3 with it.  With
    ``leaves`` given the clustering is left out and the rank matrix built in that order, as a caller does that kept the
    order: hicmi_upgma starts a pre-sort of its own, and without it hicmi_rank_matrix meets the pre-sort the context
    remembers.  Returns the leaf order."""
    if leaves is None:
        leaves, _z = ctx.upgma()
    ctx.rank_matrix(leaves)
    ctx.p2_select(SEL)
    ctx.p2_layout(STARTS, LENS)
    ctx.p2_set_arrangement(IDS, REV)
    ctx.p2_window_tables(*window_tables(3))
    return leaves


def _named(**arrays):
    return {k: np.asarray(v) for k, v in arrays.items()}


def _dep_scan(ctx):
    sig, x = ctx.cut_scan(3, ctx.n - 3, .05, want_x=True)
    return _named(sig=sig, x=x)


def _dep_filter_scan(ctx):
    sig, x = ctx.filter_scan(3, 48, 24, ctx.n - 3, .01, want_x=True)
    return _named(sig=sig, x=x)


def _dep_first_pass(ctx):
    cuts, log = ctx.first_pass_cuts(5, int(ctx.n * .95), .05)
    return _named(cuts=cuts, log=np.array(log, np.int64).reshape(-1, 2))


def _dep_filter_cuts(ctx):
    kept, warned = ctx.filter_cuts(CUTS, .05)
    return _named(kept=kept, warned=[warned])


def _dep_first_multi(ctx):
    got = {}
    _cut_lists(got, "set", ctx.first_pass_cuts_multi([(5, int(ctx.n * .95)), (9, ctx.n - 1), (14, ctx.n - 1)], .05))
    return got


def _dep_filter_multi(ctx):
    got = {}
    _cut_lists(got, "set", ctx.filter_cuts_multi([CUTS, CUTS[:2], CUTS[1:]], [.05, .01, .05]))
    return got


def _dep_table(method, *more):
    def call(ctx):
        table, best = getattr(ctx, method)(IDS, REV, *more)
        return _named(table=table, best=best)
    return call


def _dep_set_arrangement(ctx):
    """Another arrangement than the chain's, and what it adds up to: the call itself hands nothing back."""
    ctx.p2_set_arrangement(IDS[::-1], REV)
    return _named(total=[ctx.p2_arrangement_total()])


def _dep_insert_all(ctx):
    ids, rev, best = ctx.p2_insert_all(IDS, REV, NEW_IDS)
    return _named(ids=ids, rev=rev, best=[best])


def _dep_scan_arranged(ctx):
    ids, rev, best, rounds, total = ctx.p2_scan_arranged(IDS, REV, 3, *window_tables(3), 0.0)
    return _named(ids=ids, rev=rev, end=[best, rounds, total])


def _dep_shortlist(ctx):
    got = {}
    _short_lists(got, "window", ctx.p2_window_shortlist(0, 3, 3, TOTAL, 0.0, None))
    return got


# (the method, the call that rebuilds the state it answers from, how it is called)
DEPENDENTS = (
    ("raw_merges", "upgma", lambda ctx: _named(z=ctx.raw_merges())),
    ("rank_rows", "rank_matrix", lambda ctx: _named(rank=ctx.rank_rows(), inverse=ctx.rank_rows(inverse=True))),
    ("cut_scan", "rank_matrix", _dep_scan),
    ("filter_scan", "rank_matrix", _dep_filter_scan),
    ("first_pass_cuts", "rank_matrix", _dep_first_pass),
    ("filter_cuts", "rank_matrix", _dep_filter_cuts),
    ("first_pass_cuts_multi", "rank_matrix", _dep_first_multi),
    ("filter_cuts_multi", "rank_matrix", _dep_filter_multi),
    ("p2_total", "p2_select", lambda ctx: _named(total=[ctx.p2_total()])),
    ("p2_score", "p2_select", lambda ctx: _named(scores=ctx.p2_score(PERMS, TOTAL))),
    ("p2_score_exact", "p2_select", lambda ctx: _named(scores=ctx.p2_score_exact(PERMS, TOTAL))),
    ("p2_layout", "p2_select", lambda ctx: ctx.p2_layout(STARTS, LENS) or {}),
    ("p2_set_arrangement", "p2_layout", _dep_set_arrangement),
    ("p2_insert_all", "p2_layout", _dep_insert_all),
    ("p2_support", "p2_layout", _dep_table("p2_support", TOTAL)),
    ("p2_breaks", "p2_layout", _dep_table("p2_breaks", LENS[IDS], TOTAL)),
    ("p2_inversions", "p2_layout", _dep_table("p2_inversions", TOTAL)),
    ("p2_scan_arranged", "p2_layout", _dep_scan_arranged),
    ("p2_arrangement_total", "p2_set_arrangement", lambda ctx: _named(total=[ctx.p2_arrangement_total()])),
    ("p2_arrangement_score", "p2_set_arrangement", lambda ctx: _named(score=[ctx.p2_arrangement_score(TOTAL)])),
    ("p2_score_insertions", "p2_set_arrangement", lambda ctx: _named(scores=ctx.p2_score_insertions(8, TOTAL))),
    ("p2_score_window", "p2_set_arrangement", lambda ctx: _named(delta=ctx.p2_score_window(1, 3))),
    ("p2_decide_window", "p2_set_arrangement", lambda ctx: _named(decision=np.array(ctx.p2_decide_window(1, 3, TOTAL, 0.0, None)))),
    ("p2_window_shortlist", "p2_set_arrangement", _dep_shortlist),
)
# the words of the refusal of a dependent whose state is gone, by the step that would rebuild it
NOT_RUN = {"upgma": "hicmi_upgma has not run", "rank_matrix": "hicmi_rank_matrix has not run",
           "p2_select": "hicmi_p2_select has not run", "p2_layout": "hicmi_p2_layout has not run",
           "p2_set_arrangement": "hicmi_p2_set_arrangement has not run"}
# A dependent may be refused for an earlier link of the chain than its own: with the selection gone the layout is gone
REFUSALS = {"upgma": ("upgma",), "rank_matrix": ("rank_matrix",), "p2_select": ("p2_select",),
            "p2_layout": ("p2_select", "p2_layout"), "p2_set_arrangement": ("p2_select", "p2_layout", "p2_set_arrangement")}


@functools.lru_cache(maxsize=None)
def stale_maps():
    """The 192-bin map the state is built on, and another 192-bin map."""
    from hic_genome_assembler_amd import synth
    out = []
    for seed in (11, 31):
        layout = synth.make_layout(192, seed=seed)
        c = synth.dense_contacts(layout, seed=seed)
        c.setflags(write=False)
        out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stale_pairs():
    """Twelve scaffolds of 8 .. 19 bins at 500 bases a bin (162 bins), in three sequences, and 6,000 pairs on them."""
    rng = np.random.default_rng(41)
    sizes = (4000 + 500 * np.arange(12) - 37).astype(np.int64)
    chroms = [[(int(s), "+-"[s % 2]) for s in range(q, 12, 3)] for q in range(3)]
    tables = lref.layout(chroms, sizes, 100)
    sa = rng.integers(0, 12, 6000)
    sb = np.where(rng.random(6000) < .5, sa, rng.integers(0, 12, 6000))
    pa = 1 + np.floor(rng.random(6000) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(6000) * sizes[sb]).astype(np.int64)
    return sizes, tables, (sa.astype(np.int32), pa, sb.astype(np.int32), pb)


def _replace_device(ctx, donor):
    ptr, n, ld = donor.contacts_device()
    ctx.set_contacts_device(ptr, n, ld, keepalive=donor)


def _replace_map(ctx, lifted):
    sizes, tables, pairs = stale_pairs()
    if lifted:
        ctx.map_begin_lifted(sizes, *tables, 500)
    else:
        ctx.map_begin(sizes, 500)
    ctx.map_add_pairs(*pairs)
    ctx.map_finish()


def _mend_masked(ctx):
    """A map with empty rows cannot be clustered or ranked as it stands (0 / 0 in the distances; the pipeline drops such
    rows first), so sums of 1 are installed for them before the chain is rebuilt - and only then: hicmi_set_row_sums
    forgets the rank matrix and the merges itself, so what a dependent does right after hicmi_ice_mask_rows is looked at
    before this call."""
    np_sum, seq_sum = ctx.row_sums()
    ctx.set_row_sums(np.where(np_sum == 0, 1.0, np_sum), np.where(seq_sum == 0, 1.0, seq_sum))


def _replace_sums(ctx):
    """Other sums under the same matrix: np_sum scaled (the distances divide by it, so the merges change), seq_sum with
    the sign of every third row turned.  A row's similarity keys are seq_sum[i] * C[i][j] / np_sum[i], so a positive factor
    leaves the order inside the row - the rank row - as it is, and a negative one reverses it."""
    np_sum, seq_sum = ctx.row_sums()
    ctx.set_row_sums(np_sum * 1.25, np.where(np.arange(len(seq_sum)) % 3 == 1, -seq_sum, seq_sum))


# (the name, what it does to a context that holds stale_maps()[0]; ``donor`` is a context that holds stale_maps()[1])
REPLACERS = (
    ("set_contacts", lambda ctx, donor: ctx.set_contacts(stale_maps()[1])),
    ("set_contacts_f32", lambda ctx, donor: ctx.set_contacts(stale_maps()[1].astype(np.float32))),
    ("set_contacts_device", _replace_device),
    ("compact", lambda ctx, donor: ctx.compact(np.flatnonzero(np.arange(192) % 4 != 1))),
    ("rebin", lambda ctx, donor: ctx.rebin(np.arange(0, 193, 2))),
    ("map_finish", lambda ctx, donor: _replace_map(ctx, False)),
    ("map_finish_lifted", lambda ctx, donor: _replace_map(ctx, True)),
    ("ice_mask_rows", lambda ctx, donor: ctx.ice_mask_rows((np.arange(192) % 5 == 2).astype(np.uint8))),
    ("ice_balance", lambda ctx, donor: ctx.ice_balance(max_iter=8)),
    ("set_row_sums", lambda ctx, donor: _replace_sums(ctx)),
)
# what each replacer leaves standing: set_row_sums keeps the matrix, and with it all of Part 2
KEEPS = {"set_row_sums": ("p2_select", "p2_layout", "p2_set_arrangement")}
# what has to follow a replacer before the chain can be rebuilt on the matrix it leaves (after the dependents were asked)
MENDS = {"ice_mask_rows": _mend_masked}


def mend(replacer, ctx):
    MENDS.get(replacer, lambda ctx: None)(ctx)


class _Marks:
    """What a binding hands to the library in one call: the arrays it allocates with numpy.empty come pre-filled with the
    byte 0xA5, every array is photographed at the moment its address is taken (_lib._ptr: outputs made with numpy.zeros
    and the arrays that are input and output at once included), and every int64 and double scalar when it is made."""

    def __init__(self):
        self.filled, self.arrays, self.scalars = [], [], []

    def __getattr__(self, name):                            # (stands in for numpy inside the binding)
        return getattr(np, name)

    def empty(self, shape, dtype=float, **kw):
        a = np.empty(shape, dtype, **kw)
        a.view(np.uint8).reshape(-1)[:] = 0xA5
        self.filled.append(a)
        return a

    def untouched(self):
        return (all((a.view(np.uint8) == 0xA5).all() for a in self.filled)
                and all(a.tobytes() == image for a, image in self.arrays)
                and all(bytes(x) == image for x, image in self.scalars))


@contextlib.contextmanager
def marked_outputs():
    """Inside: whatever the binding passes to the library - arrays and scalars - is recorded as it is at the call; the
    object yielded says afterwards whether the library left all of it as it was."""
    import ctypes
    from hic_genome_assembler_amd import _lib
    marks = _Marks()
    real = (_lib.np, _lib._ptr, _lib.c_i64, _lib.c_dbl)

    def ptr(a):
        if a is not None:
            marks.arrays.append((a, a.tobytes()))
        return real[1](a)

    def recorded(kind):
        class Recorded(kind):
            def __init__(self, *value):
                kind.__init__(self, *value)
                marks.scalars.append((self, bytes(self)))
        return Recorded

    _lib.np, _lib._ptr, _lib.c_i64, _lib.c_dbl = marks, ptr, recorded(ctypes.c_int64), recorded(ctypes.c_double)
    try:
        yield marks
    finally:
        _lib.np, _lib._ptr, _lib.c_i64, _lib.c_dbl = real


# ---- the tables held against the source (tests/test_reuse_cpu.py) ------------------------------------------------------------
# Every DevBuf<> and PinBuf<> member of struct hicmi_ctx (the observation matrix of an HMM slot as "hslot.d_x"): the
# families whose cases make it regrow - their second case for the matrix families, their third for the pair families.
_P1, _TAB, _SRCH = ("part1",), ("p2_tables",), ("p2_search",)
BUFFERS = {
    "c_own": ("part1", "ice", "rebin", "buildmap", "liftmap"), "d_np": _P1 + ("rebin",), "d_seq": _P1 + ("rebin",),
    "dW": _P1, "dW2": _P1, "d_size": _P1, "d_chain": _P1, "d_status": _P1, "d_zraw": _P1,
    "d_order": _P1, "dR": _P1, "dRank": _P1, "d_sort_scratch": _P1, "dRankS": _P1, "d_ident": _P1, "d_ties": _P1,
    "d_tie_bits": _P1, "d_row_list": _P1, "d_x": _P1, "d_sig": _P1, "d_scan_multi": _P1, "d_tmp": _P1,
    "dM2": _TAB + _SRCH, "d_sel": _TAB + _SRCH, "d_H": _TAB + _SRCH, "d_perms": _SRCH, "d_scores": _SRCH, "d_partial": _SRCH,
    "d_T": _TAB + _SRCH, "d_scaf_start": _TAB + _SRCH, "d_scaf_len": _TAB + _SRCH, "d_arr_packed": _TAB + _SRCH,
    "d_pos2sel": _TAB + _SRCH, "d_orders": _SRCH, "d_orients": _SRCH, "d_G": _SRCH, "d_delta": _SRCH, "d_wb": _SRCH,
    "d_wnear": _SRCH, "d_arr_packed2": _SRCH, "d_pos2sel2": _SRCH, "d_ins_T": _SRCH, "d_ins_partial": _TAB + _SRCH,
    "d_ins_blob": _SRCH, "d_ins_steps": _SRCH, "d_sup_recs": _TAB, "d_brk_recs": _TAB, "d_inv_recs": _TAB,
    "d_gs_lists": ("group_junction",), "d_gs_sums": ("group_junction",), "d_jn_lists": ("group_junction",),
    "d_jn_sums": ("group_junction",), "d_ice": ("ice",), "d_ice_mask": ("ice",),
    "hslot.d_x": ("hmm",), "d_hmulti": ("hmm",), "d_horder": ("hmm",), "d_hwork": ("hmm",), "d_hlab": ("hmm",),
    "d_hbt": ("hmm",), "d_hpart": ("hmm",), "d_hsmall": ("hmm",), "d_hhist": ("hmm",), "d_hst": ("hmm",),
    "d_lvA": ("louvain",), "d_lvvec": ("louvain",), "d_lvrows": ("louvain",), "d_lvwork": ("louvain",),
    "map_cells": ("buildmap", "liftmap"), "d_map_first": ("buildmap", "liftmap"),
    "d_map_chunk": ("buildmap", "liftmap", "spans", "ends", "anchor", "split", "pairs_store"), "d_map_lift": ("liftmap",),
    "d_stat_lift": ("liftmap",), "d_stat_out": ("liftmap",),
    "span_marks": ("spans",), "d_span_lift": ("spans",), "d_span_first": ("spans",),
    "ends_table": ("ends", "resident"), "d_ends_lift": ("ends", "resident"), "d_ends_rank": ("ends", "resident"),
    "anchor_table": ("anchor", "resident"), "d_anchor_lift": ("anchor", "resident"), "d_anchor_first": ("anchor", "resident"),
    "d_anchor_target": ("anchor", "resident"),
    "seats_table": ("resident",), "d_seats_lift": ("resident",), "d_seats_first": ("resident",), "d_seats_rank": ("resident",),
    "d_links_table": ("resident",), "d_links_recs": ("resident",), "d_links_size": ("resident",), "d_links_lift": ("resident",),
    "d_links_seq_size": ("resident",),
    "d_pairs_scaf_a": ("pairs_store", "resident"), "d_pairs_scaf_b": ("pairs_store", "resident"),
    "d_pairs_pos_a": ("pairs_store", "resident"), "d_pairs_pos_b": ("pairs_store", "resident"),
    "d_pairs_intra": ("pairs_store", "resident"), "d_pairs_work": ("pairs_store", "resident"),
    "pin_pairs_len": ("pairs_store", "resident"),
    "d_plot_order": ("plot",), "d_plot_work": ("plot",), "d_plot_img": ("plot",),
    "pin_up": tuple(FAMILIES), "pin_down": tuple(FAMILIES),
}
# Every function of the driver that drops or installs a matrix, says that the matrix changed, assigns dC or uploads into
# d_np, with the replacers that reach it.
_ALL_BUT_SUMS = tuple(name for name, _f in REPLACERS if name != "set_row_sums")
REPLACER_SITES = {
    "drop_matrix_state": tuple(n for n in _ALL_BUT_SUMS if not n.startswith("ice_")),
    "own_matrix": ("compact", "rebin", "map_finish", "map_finish_lifted"),
    "hicmi_set_contacts_host": ("set_contacts",),
    "hicmi_set_contacts_host_f32": ("set_contacts_f32",),
    "hicmi_set_contacts_device": ("set_contacts_device",),
    "hicmi_set_row_sums": ("set_row_sums",),
    "hicmi_compact": ("compact",),
    "hicmi_rebin": ("rebin",),
    "map_install": ("map_finish", "map_finish_lifted"),
    "ice_matrix_changed": ("ice_mask_rows", "ice_balance"),
    "hicmi_ice_mask_rows": ("ice_mask_rows",),
    "hicmi_ice_balance": ("ice_balance",),
}
