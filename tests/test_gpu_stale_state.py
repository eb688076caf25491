"""What a new matrix invalidates (include/hicmi.h, the contact-matrix section).  For every call that puts
another matrix or other sums under a context (rc.REPLACERS) and every method that answers from state derived from the
matrix (rc.DEPENDENTS): with the state built on one 192-bin map and the replacer applied with another, the dependent
either refuses - "... has not run", naming a missing step, and writes nothing - or gives the bytes a fresh context gives
for what the context holds now.  It never gives the old answer.  Rebuilding the chain then gives the fresh context's
bytes.  The snapshots - copies that are documented to survive - come back bit for bit after every replacer, and a build
that was open across it finishes to the result it gives undisturbed."""
import numpy as np
import pytest

import reuse_cases as rc

pytestmark = pytest.mark.gpu

PAIRS = [(r[0], d[0]) for r in rc.REPLACERS for d in rc.DEPENDENTS]
_fresh = {}
_undisturbed = {}


@pytest.fixture(autouse=True)
def _default_forms(monkeypatch):
    rc.default_forms(monkeypatch)


@pytest.fixture(scope="module")
def contexts():
    """The context under test, reused by every case (each starts from set_contacts), and one that holds the other map for
    set_contacts_device to adopt."""
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx, _lib.Context(0) as donor:
        donor.set_contacts(rc.stale_maps()[1])
        yield ctx, donor


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for key in want:
        a, b = np.asarray(got[key]), np.asarray(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, key)
        assert a.tobytes() == b.tobytes(), "%s: %s is not what a fresh context gives" % (what, key)


def _image(got):
    return {key: (str(np.asarray(a).dtype), np.asarray(a).shape, np.asarray(a).tobytes()) for key, a in got.items()}


def _fresh_after(replacer, donor):
    """{dependent: its answer} on a context that never held derived state of the first map: the replacer applied to a
    context that holds nothing but that map, then the chain built before every dependent (some of them move the
    arrangement)."""
    from hic_genome_assembler_amd import _lib
    if replacer not in _fresh:
        with _lib.Context(0) as ctx:
            ctx.set_contacts(rc.stale_maps()[0])
            dict(rc.REPLACERS)[replacer](ctx, donor)
            rc.mend(replacer, ctx)
            assert ctx.n >= 96
            out = {}
            for name, _step, call in rc.DEPENDENTS:
                out["leaves"] = rc.build_chain(ctx)
                out[name] = call(ctx)
            _fresh[replacer] = out
    return _fresh[replacer]


def test_the_product_is_whole():
    """Every replacer with every dependent, none left out or marked: about 250 calls on maps of at most 192 bins."""
    assert len(PAIRS) == len(rc.REPLACERS) * len(rc.DEPENDENTS) == len(set(PAIRS)) >= 240
    assert {step for _n, step, _c in rc.DEPENDENTS} == set(rc.CHAIN) == set(rc.NOT_RUN) == set(rc.REFUSALS)


@pytest.mark.parametrize("replacer,dependent", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_no_dependent_answers_for_a_matrix_that_is_gone(replacer, dependent, contexts):
    from hic_genome_assembler_amd import _lib
    ctx, donor = contexts
    step, call = {name: (step, call) for name, step, call in rc.DEPENDENTS}[dependent]
    want = _fresh_after(replacer, donor)[dependent]
    ctx.set_contacts(rc.stale_maps()[0])
    rc.build_chain(ctx)
    old = call(ctx)                                            # (the state is there and answers)
    # (balancing the synthetic map, which is balanced as it comes, scales its rows too little to reorder one)
    bites = ("raw_merges", "p2_total", "p2_arrangement_total") + (("rank_rows",) if replacer != "ice_balance" else ())
    if dependent in bites and step not in rc.KEEPS.get(replacer, ()):
        assert _image(old) != _image(want), "%s does not change what %s answers: the case shows nothing" % (replacer, dependent)
    rc.build_chain(ctx)
    dict(rc.REPLACERS)[replacer](ctx, donor)
    refusal = None
    with rc.marked_outputs() as marks:
        try:
            got = call(ctx)
        except _lib.HicmiError as e:
            refusal = str(e)
    if refusal is not None:
        assert any(rc.NOT_RUN[s] in refusal for s in rc.REFUSALS[step]), refusal
        assert marks.untouched(), "%s was refused after %s and wrote into its outputs" % (dependent, replacer)
        assert step not in rc.KEEPS.get(replacer, ()), "%s keeps what %s answers from" % (replacer, dependent)
    else:
        assert _image(got) == _image(want) or _image(got) != _image(old), \
            "%s after %s: the answer of the matrix that is gone" % (dependent, replacer)
        _same(got, want, "%s after %s, before anything was rebuilt" % (dependent, replacer))
    # rebuilt as a caller does that knows the leaf order of the new matrix: without a clustering, except for its merges
    rc.mend(replacer, ctx)
    rc.build_chain(ctx, None if step == "upgma" else _fresh_after(replacer, donor)["leaves"])
    _same(call(ctx), want, "%s after %s and a rebuilt chain" % (dependent, replacer))


# ---- snapshots ------------------------------------------------------------------------------------------------------------------
def _open_builds(ctx, case, with_map):
    """A span, an ends and an anchor build (and a map build) opened with the first half of the pairs."""
    first, _second = case.chunks(2)
    out = {"cell_first": ctx.span_begin(case.sizes, *case.tables, rc.STEP, 0)}
    ctx.span_add_pairs(*first)
    out["rank"] = ctx.ends_begin(case.sizes, *case.tables, rc.WINDOW, rc.REACH)
    ctx.ends_add_pairs(*first)
    out["anchor_first"] = ctx.anchor_begin(case.sizes, *case.dropped, case.rank_target(), rc.WINDOW)
    ctx.anchor_add_pairs(*first)
    if with_map:
        ctx.map_begin(case.sizes, 1500)
        ctx.map_add_pairs(*first)
    return out


def _finish_builds(ctx, case, with_map, out):
    _first, second = case.chunks(2)
    ctx.span_add_pairs(*second)
    out["picks"], out["span_counters"], out["depth"] = ctx.span_finish(rc.FLANK, rc.span_records(case))
    ctx.ends_add_pairs(*second)
    out["ends_table"], out["ends_counters"] = ctx.ends_finish()
    ctx.anchor_add_pairs(*second)
    out["anchor_table"], out["anchor_counters"] = ctx.anchor_finish()
    if with_map:
        ctx.map_add_pairs(*second)
        out["map_pairs"] = np.array([ctx.map_finish()])
        out["map"] = ctx.contacts_host()
    return out


def _builds_undisturbed(case, with_map):
    from hic_genome_assembler_amd import _lib
    if with_map not in _undisturbed:
        with _lib.Context(0) as ctx:
            ctx.set_contacts(rc.stale_maps()[0])
            _undisturbed[with_map] = _finish_builds(ctx, case, with_map, _open_builds(ctx, case, with_map))
    return _undisturbed[with_map]


def _links_rows(ctx, n_rows):
    """The rows of the last links call, fetched again (hicmi_links_fetch alone: nothing is recomputed)."""
    from hic_genome_assembler_amd import _lib
    lo, hi, counts = np.zeros(n_rows, np.int32), np.zeros(n_rows, np.int32), np.zeros((n_rows, 5), np.uint64)
    _lib._check(ctx._lib.hicmi_links_fetch(ctx._h, _lib._ptr(lo), _lib._ptr(hi), _lib._ptr(counts)))
    return lo, hi, counts


def _snapshots(ctx, n_rows):
    got = {}
    for slot in (0, 1):
        ctx.hmm_use_obs(slot)
        got["obs%d" % slot] = ctx.hmm_get_obs()
    got["A"], got["gdegrees"], total_weight = ctx.louvain_get_graph()
    got["total_weight"] = np.array([total_weight])
    n_kept, n_intra, got["intra"] = ctx.pairs_info()
    got["pairs_info"] = np.array([n_kept, n_intra])
    got["scaf_a"], got["pos_a"], got["scaf_b"], got["pos_b"] = ctx.pairs_fetch()
    got["links_lo"], got["links_hi"], got["links_counts"] = _links_rows(ctx, n_rows)
    return got


@pytest.mark.parametrize("replacer", [r[0] for r in rc.REPLACERS])
def test_snapshots_survive_and_open_builds_finish_undisturbed(replacer, contexts):
    ctx, donor = contexts
    case = rc.pair_cases()[1]
    with_map = not replacer.startswith("map_finish")           # (those two open and finish a map build themselves)
    want_builds = _builds_undisturbed(case, with_map)
    ctx.set_contacts(rc.stale_maps()[0])
    ctx.row_sums()
    rc.build_chain(ctx)
    leaves, _z = ctx.upgma(want_linkage=False)
    ctx.hmm_load_obs(leaves, 24, 96)
    ctx.hmm_load_obs_slot(1, leaves, 48, 64)
    ctx.louvain_graph(np.arange(0, 192, 2, dtype=np.int32))
    rc.load_store(ctx, case)
    try:
        lo, _hi, _counts, _counters = ctx.links_resident(case.sizes, rc.WINDOW)
        assert len(lo) >= 4
        builds = _open_builds(ctx, case, with_map)
        before = _snapshots(ctx, len(lo))
        dict(rc.REPLACERS)[replacer](ctx, donor)
        _same(_snapshots(ctx, len(lo)), before, "the snapshots after " + replacer)
        _same(_finish_builds(ctx, case, with_map, builds), want_builds, "the builds open across " + replacer)
    finally:
        ctx.pairs_drop()
    # the window tables are a copy too: with the chain rebuilt up to the arrangement and the tables not loaded again, the
    # windows of the new matrix are scored with them
    if with_map:
        ctx.set_contacts(rc.stale_maps()[0])
        dict(rc.REPLACERS)[replacer](ctx, donor)
    rc.mend(replacer, ctx)
    leaves, _z = ctx.upgma()
    ctx.rank_matrix(leaves)
    ctx.p2_select(rc.SEL)
    ctx.p2_layout(rc.STARTS, rc.LENS)
    ctx.p2_set_arrangement(rc.IDS, rc.REV)
    call = {name: call for name, _step, call in rc.DEPENDENTS}["p2_score_window"]
    _same(call(ctx), _fresh_after(replacer, donor)["p2_score_window"], "the window tables after " + replacer)


def test_a_new_selection_forgets_the_exact_scores_of_the_last():
    """hicmi_p2_select is to Part 2 what a replacer is to the context: the literal scores cached by bin order under one
    total belong to the selection they were computed on.  Two selections of the same size on one map, the same layout,
    arrangement and total: the decisions on the second are those of a context that never saw the first."""
    from hic_genome_assembler_amd import _lib

    def decisions(ctx, sel):
        ctx.p2_select(sel)
        ctx.p2_layout(rc.STARTS, rc.LENS)
        ctx.p2_set_arrangement(rc.IDS, rc.REV)
        ctx.p2_window_tables(*rc.window_tables(3))
        got = {"window": np.array(ctx.p2_decide_window(1, 3, rc.TOTAL, 0.0, None))}
        ids, rev, best = ctx.p2_insert_all(rc.IDS, rc.REV, rc.NEW_IDS)
        got.update(ids=ids, rev=rev, best=np.array([best]))
        return got

    with _lib.Context(0) as ctx:
        ctx.set_contacts(rc.stale_maps()[0])
        first = decisions(ctx, rc.SEL)
        second = decisions(ctx, rc.SEL + 100)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(rc.stale_maps()[0])
        want = decisions(ctx, rc.SEL + 100)
    assert _image(first) != _image(want)
    _same(second, want, "the second selection")
