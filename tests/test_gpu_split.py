"""Read pairs moved to the pieces of cut scaffolds on the device (hicmi_split_pairs, hicmi_split_maps) against
tests/split_reference.py, for HICMI_SPLIT_PLAIN unset, =1 and =0.  Pieces, positions, counters and maps are integers, so
every comparison is exact: there are no tolerances.  The maps are also held to hicmi_build_maps on the rewritten pair file
and, lifted back onto the parents, to hicmi_build_maps on the original one; then the command line end to end."""
import functools
import os
import re

import numpy as np
import pytest

import buildmap_reference as bref
import split_reference as ref

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -5
# Both kernel forms give the same bits by design: these tests hold each to the reference but cannot tell which kernel ran; that
# the switch is read per call is checked from the source in tests/test_split_cpu.py.
FORMS = {"default": {}, "plain": {"HICMI_SPLIT_PLAIN": "1"}, "combine": {"HICMI_SPLIT_PLAIN": "0"}}
FORM_NAMES = ["default", "plain", "combine"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constant(name):
    with open(os.path.join(ROOT, "hic_genome_assembler_amd", "csrc", "hicmi_internal.h")) as fh:
        text = fh.read()
    value = re.search(r"static constexpr int %s = ([^;]+);" % name, text).group(1)
    return 1 << _constant(value.split("<<")[1].strip()) if "<<" in value else int(value)


SLICE, SLOTS, MAX_BLOCKS = (_constant(k) for k in ("SPLIT_SLICE", "SPLIT_SLOTS", "SPLIT_MAX_BLOCKS"))
# the grid of either form is at most MAX_BLOCKS workgroups, a workgroup of the combining form takes SLICE pairs at a time:
# the last count makes the stride loop of both run a second time
COUNTS = [0, 1, 255, 256, 257, SLICE - 1, SLICE + 1, MAX_BLOCKS * SLICE + 5]


def _set_form(monkeypatch, form):
    for key in ("HICMI_SPLIT_PLAIN", "HICMI_BUILDMAP_CHUNK_PAIRS", "HICMI_BUILDMAP_PLAIN", "HICMI_LIFTMAP_PLAIN", "HICMI_SPANS_PLAIN"):
        monkeypatch.delenv(key, raising=False)
    for key, value in FORMS[form].items():
        monkeypatch.setenv(key, value)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _case():
    """Scaffolds of 1, 2, 3, 64 and 65 pieces, one of one base, one without a base, one above 2^33 bases cut around 2^32 and
    into pieces of one base at either end."""
    top = 2 ** 33 + 70
    sizes = np.array([50, 50, 1, 0, 50, 200, 200, top, 9, 70000], np.int64)
    cuts = {1: [25], 4: [1, 49], 5: list(range(3, 3 * 64, 3)), 6: list(range(2, 2 * 65, 2)),
            7: [1, 2 ** 31 - 5, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, top - 1], 8: [1, 8]}      # the piece after 2^32 + 1 is longer than 2^32
    first, start, size, _parent = ref.make_pieces(sizes, cuts)
    assert np.diff(first).tolist() == [1, 2, 1, 1, 3, 64, 65, 8, 3, 1]
    return (cuts,) + _frozen(sizes, first, start, size)


@functools.lru_cache(maxsize=None)
def _pool():
    """COUNTS[-1] pairs on the case: seven in ten inside one scaffold, ordered by scaffold as a HiC-Pro file is."""
    _cuts, sizes, _first, _start, _size = _case()
    rng = np.random.default_rng(11)
    n = COUNTS[-1]
    have = np.flatnonzero(sizes > 0)
    sa = np.sort(rng.choice(have, n))
    sb = rng.choice(have, n)
    cis = rng.random(n) < 0.7
    sb[cis] = sa[cis]
    pa = 1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64)
    return _frozen(sa.astype(np.int32), pa, sb.astype(np.int32), pb)


def _first_n(pairs, n):
    return tuple(a[:n] for a in pairs)


@functools.lru_cache(maxsize=None)
def _want_pool(n):
    _cuts, sizes, first, start, _size = _case()
    pairs = _first_n(_pool(), n)
    return _frozen(*ref.split_pairs(pairs, sizes, first, start)) + _frozen(ref.counters(pairs, sizes, first, start))


def _same(got, want):
    for g, w, dtype in zip(got, want, (np.int32, np.int64, np.int32, np.int64, np.uint64)):
        assert g.dtype == dtype and g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w, dtype).tobytes()


def _run(pairs, sizes, first, start, into=None):
    from hic_genome_assembler_amd import _lib
    with _lib.Context(0) as ctx:
        return ctx.split_pairs(*pairs, sizes, first, start, into=into)


# ---- hicmi_split_pairs ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("n", COUNTS)
def test_pair_counts_at_the_workgroup_slice_and_grid_edges(n, form, monkeypatch):
    _cuts, sizes, first, start, _size = _case()
    want = _want_pool(n)
    if n == COUNTS[-1]:
        assert n > MAX_BLOCKS * SLICE and n > MAX_BLOCKS * 256 and (want[4] > 0).sum() > 300
    _set_form(monkeypatch, form)
    _same(_run(_first_n(_pool(), n), sizes, first, start), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_every_cut_edge_and_piece_count(form, monkeypatch):
    """Ends at 1, c, c + 1 and L of every cut, every end against every end: scaffolds of 1, 2, 3, 64 and 65 pieces, pieces of
    one base, positions above 2^32."""
    cuts, sizes, first, start, _size = _case()
    ends = ref.edge_ends(sizes, cuts)
    assert (7, 2 ** 32 + 2) in ends and (7, int(sizes[7])) in ends and (4, 2) in ends and (2, 1) in ends and len(ends) > 250
    pairs = ref.all_pairs(ends)
    want = ref.split_pairs(pairs, sizes, first, start) + (ref.counters(pairs, sizes, first, start),)
    assert (want[1] > 2 ** 32).any() and (np.asarray(pairs[1]) - want[1] > 2 ** 32).any() and want[4][3].any()
    _set_form(monkeypatch, form)
    _same(_run(pairs, sizes, first, start), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_hot_counters_are_exact(form, monkeypatch):
    """100,000 copies of one pair inside one piece, then of one pair between two sibling pieces: the worst contention."""
    _cuts, sizes, first, start, _size = _case()
    for pa, pb, kinds in ((4, 5, [0]), (4, 120, [1, 3])):
        pairs = tuple(np.full(100000, v, dtype=t) for v, t in ((5, np.int32), (pa, np.int64), (5, np.int32), (pb, np.int64)))
        want = ref.split_pairs(pairs, sizes, first, start) + (ref.counters(pairs, sizes, first, start),)
        assert sorted(set(np.nonzero(want[4])[0].tolist())) == kinds and set(want[4][kinds[0]].tolist()) == {0, 100000}
        _set_form(monkeypatch, form)
        _same(_run(pairs, sizes, first, start), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_a_slice_with_more_counters_than_the_table_holds(form, monkeypatch):
    """Pair k lies in the pieces 2 k and 2 k + 1 of one scaffold: four counters of its own.  A slice of the combining form
    meets 4 x SLICE distinct counters, more than its table has, so contributions fall back to direct atomic adds."""
    n = SLICE + 1000
    assert 4 * SLICE > SLOTS
    sizes = np.array([7, 2 * n], np.int64)
    first, start, _size, _parent = ref.make_pieces(sizes, {1: range(1, 2 * n)})
    k = np.arange(n, dtype=np.int64)
    pairs = (np.ones(n, np.int32), 2 * k + 1, np.ones(n, np.int32), 2 * k + 2)
    want = ref.split_pairs(pairs, sizes, first, start) + (ref.counters(pairs, sizes, first, start),)
    assert want[4][1].tolist() == [0] + [1] * (2 * n) and want[4][3].tolist() == [0] + [1, 2 ** 64 - 1] * n
    _set_form(monkeypatch, form)
    _same(_run(pairs, sizes, first, start), want)


@pytest.mark.parametrize("form", FORM_NAMES)
def test_counters_are_added_and_two_calls_equal_one(form, monkeypatch):
    from hic_genome_assembler_amd import _lib
    _cuts, sizes, first, start, _size = _case()
    n = 5000
    pairs, want = _first_n(_pool(), n), _want_pool(n)
    _set_form(monkeypatch, form)
    held = (np.arange(4 * len(start), dtype=np.uint64) * np.uint64(2 ** 60 + 3)).reshape(4, -1)      # wraps: the adds are mod 2^64
    into = held.copy()
    with _lib.Context(0) as ctx:
        parts = [ctx.split_pairs(*tuple(a[lo:hi] for a in pairs), sizes, first, start, into=into) for lo, hi in ((0, 1234), (1234, n))]
        assert parts[0][4] is into and parts[1][4] is into and into.tobytes() == (held + want[4]).tobytes()
        _same(tuple(np.concatenate([a, b]) for a, b in zip(parts[0][:4], parts[1][:4])) + (into - held,), want)


def test_misuse_changes_nothing_and_leaves_open_builds_intact(monkeypatch):
    from hic_genome_assembler_amd import _lib
    import liftmap_reference as lref
    _set_form(monkeypatch, "default")
    _cuts, sizes, first, start, _size = _case()
    n = 5000
    pairs, want = _first_n(_pool(), n), _want_pool(n)
    sa, pa, sb, pb = pairs
    lib = _lib.load()
    held = np.arange(25, dtype=np.float64).reshape(5, 5)
    held = held + held.T
    small = np.minimum(sizes, 10 ** 6)                                         # the builds that stay open: scaffolds of at most 1 Mb
    small_pairs = (sa, np.minimum(pa, small[sa]), sb, np.minimum(pb, small[sb]))
    tables = lref.identity(small)

    def changed(arr, at, value):
        out = np.array(arr)
        out[at] = value
        return out

    def call(ctx, sa=sa, pa=pa, sb=sb, pb=pb, sizes=sizes, first=first, start=start):
        outs = [np.full(n, -7, np.int32), np.full(n, -7, np.int64), np.full(n, -7, np.int32), np.full(n, -7, np.int64),
                np.full((4, len(start)), 77, np.uint64)]
        size, f, s = _lib._split_tables(sizes, first, start)
        arrays = [np.ascontiguousarray(a, t) for a, t in ((sa, np.int32), (pa, np.int64), (sb, np.int32), (pb, np.int64))]
        rc = lib.hicmi_split_pairs(ctx._h, *[_lib._ptr(a) for a in arrays], n, _lib._ptr(size), len(size), _lib._ptr(f), _lib._ptr(s),
                                   len(s), *[_lib._ptr(o) for o in outs])
        return rc, outs, lib.hicmi_last_error().decode()

    def unwritten(outs):
        return all((o == -7).all() for o in outs[:4]) and (outs[4] == 77).all()

    with _lib.Context(0) as ctx:
        ctx.set_contacts(held)
        ctx.map_begin(small, 1000)                                              # a map build and a span build stay open through all of this
        ctx.map_add_pairs(*_first_n(small_pairs, 2000))
        ctx.span_begin(small, *tables, 500)
        ctx.span_add_pairs(*_first_n(small_pairs, 2000))
        for kwargs, word in (({"sa": changed(sa, 200, len(sizes))}, "pair 200 "), ({"sb": changed(sb, 4999, -1)}, "pair 4999 "),
                             ({"pa": changed(pa, 0, 0)}, "pair 0 "), ({"pb": changed(pb, 100, sizes[sb[100]] + 1)}, "pair 100 "),
                             ({"start": changed(start, 2, 0)}, "scaffold 1"), ({"first": changed(first, 3, 5)}, "scaffold 2"),
                             ({"sizes": changed(sizes, 5, 100)}, "scaffold 5")):
            rc, outs, message = call(ctx, **kwargs)
            assert rc == EINVAL and word in message and unwritten(outs), message
        rc, outs, message = call(ctx)
        assert rc == 0
        _same(outs[:4] + [outs[4] - np.uint64(77)], want)
        assert ctx.n == 5 and ctx.contacts_host().tobytes() == held.tobytes()
        # the two builds that were open all the while take the rest of their pairs and are what they would have been
        ctx.span_add_pairs(*tuple(a[2000:] for a in small_pairs))
        import span_reference as sref
        D, counters, _marks = sref.depth(small_pairs, small, tables, 500)
        _picks, got_counters, got_D = ctx.span_finish(1, np.zeros((0, 4), np.int64))
        assert got_D.tobytes() == D.tobytes() and got_counters.tolist() == counters.tolist()
        ctx.map_add_pairs(*tuple(a[2000:] for a in small_pairs))
        assert ctx.map_finish() == n and ctx.contacts_host().tobytes() == bref.build(small_pairs, small, 1000).tobytes()


# ---- hicmi_split_maps ------------------------------------------------------------------------------------------------------------
RESOLUTIONS = [1000, 2500, 333]


@functools.lru_cache(maxsize=None)
def _file_case():
    """12 scaffolds, 5 of them cut, and a 2,000-line file with CRLF lines, 6 and 12 columns, skipped lines of both kinds."""
    names = ["ctg%d" % (k + 1) for k in range(12)]
    sizes = np.array([5000, 1, 999, 12000, 3007, 8000, 700, 30000, 1000, 1001, 6400, 2500], np.int64)
    cuts = {0: [2500], 3: [1000, 1001, 11999], 4: [3006], 7: [1, 333, 666, 7000, 7001], 11: [1250]}
    first, start, size, parent = ref.make_pieces(sizes, cuts)
    data = bref.odd_file_bytes(names, sizes, 2000, seed=41)
    pairs, stats, _after = bref.parse_text(data, names, sizes)
    assert stats[2] > 50 and stats[3] > 50 and stats[1] > 1500
    moved = ref.split_pairs(pairs, sizes, first, start)
    maps = tuple(bref.build(moved, size, r) for r in RESOLUTIONS)
    counters = ref.counters(pairs, sizes, first, start)
    _frozen(sizes, first, start, size, parent, counters, *maps)
    return {"names": names, "sizes": sizes, "first": first, "start": start, "piece_sizes": size, "parent": parent,
            "piece_names": ref.piece_names(names, first), "data": data, "pairs": pairs, "stats": stats, "maps": maps, "counters": counters}


def _write(tmp_path, data, name="pairs.allValidPairs"):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def _split_maps(case, path, resolutions, ctxs, **kw):
    from hic_genome_assembler_amd import _lib
    return _lib.split_maps(path, case["names"], case["sizes"], case["first"], case["start"], resolutions, ctxs, **kw)


@pytest.mark.parametrize("form", FORM_NAMES)
@pytest.mark.parametrize("chunk", ["7", "256", None])
def test_split_maps_equal_the_reference_and_build_maps_on_the_rewritten_file(chunk, form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    case = _file_case()
    path = _write(tmp_path, case["data"])
    _set_form(monkeypatch, form)
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    stats = case["stats"]
    ctxs = [_lib.Context(0) for _r in RESOLUTIONS]
    others = [_lib.Context(0) for _r in RESOLUTIONS]
    try:
        got, counters = _split_maps(case, path, RESOLUTIONS, ctxs, threads=3)
        assert got[:4] == stats and got[4] == (-(-stats[1] // int(chunk)) if chunk else 1)
        assert counters.dtype == np.uint64 and counters.tobytes() == case["counters"].tobytes()
        for ctx, want in zip(ctxs, case["maps"]):
            assert ctx.n == len(want) and ctx.contacts_host().tobytes() == want.tobytes()
            assert np.triu(want).sum() == stats[1]
        # an independent path through code that was there before: the rewritten file counted on the pieces as scaffolds
        rewritten = str(tmp_path / "split.allValidPairs")
        assert _lib.split_valid_pairs(path, rewritten, case["names"], case["sizes"], case["first"], case["start"],
                                      case["piece_names"], threads=3) == stats
        monkeypatch.delenv("HICMI_BUILDMAP_CHUNK_PAIRS", raising=False)
        assert _lib.build_maps(rewritten, case["piece_names"], case["piece_sizes"], RESOLUTIONS, others)[:4] == (stats[1], stats[1], 0, 0)
        for ctx, other in zip(ctxs, others):
            assert ctx.contacts_host().tobytes() == other.contacts_host().tobytes()
    finally:
        for ctx in ctxs + others:
            ctx.close()


@pytest.mark.parametrize("form", FORM_NAMES)
def test_no_resolution_gives_the_counters_alone_and_adds_them(form, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    case = _file_case()
    path = _write(tmp_path, case["data"])
    _set_form(monkeypatch, form)
    monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", "500")
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    held = held + held.T
    with _lib.Context(0) as ctx:
        ctx.set_contacts(held)
        got, counters = _split_maps(case, path, [], [ctx])
        assert got[:4] == case["stats"] and got[4] == -(-case["stats"][1] // 500) and counters.tobytes() == case["counters"].tobytes()
        again = _split_maps(case, path, [], [ctx], into=counters)[1]
        assert again is counters and counters.tobytes() == (case["counters"] * np.uint64(2)).tobytes()
        assert ctx.n == 4 and ctx.contacts_host().tobytes() == held.tobytes()
        with pytest.raises(_lib.HicmiError):
            ctx.map_finish()                                                  # no build is left open


@pytest.mark.parametrize("chunk", ["256", None])
def test_split_maps_error_changes_no_context_and_no_counter(chunk, tmp_path, monkeypatch):
    from hic_genome_assembler_amd import _lib
    case = _file_case()
    _set_form(monkeypatch, "default")
    if chunk:
        monkeypatch.setenv("HICMI_BUILDMAP_CHUNK_PAIRS", chunk)
    data = case["data"] + b"\n"
    bad = _write(tmp_path, data + b"read\tctg4\t12x\t+\tctg4\t5\n", "bad.allValidPairs")
    held = np.arange(16, dtype=np.float64).reshape(4, 4)
    held = held + held.T
    into = _lib.new_split_counters(len(case["start"]))
    missing = str(tmp_path / "missing")

    def refused(call, code, word):
        with pytest.raises(_lib.HicmiError) as exc:
            call()
        assert "error %d:" % code in str(exc.value) and word in str(exc.value), str(exc.value)

    with _lib.Context(0) as a, _lib.Context(0) as b:
        a.set_contacts(held)

        def unchanged():
            assert a.n == 4 and a.contacts_host().tobytes() == held.tobytes() and not into.any()
            for call in (b.contacts_device, a.map_finish, b.map_finish):         # b has no matrix, and no build is left open
                with pytest.raises(_lib.HicmiError):
                    call()

        refused(lambda: _split_maps(case, bad, [1000, 2500], [a, b], into=into), EINVAL, "at byte %d" % len(data))
        unchanged()
        # refused before the file is opened: a resolution with more than 65,536 bins (70,608 bases), bad tables
        refused(lambda: _split_maps(case, missing, [1000, 1], [a, b], into=into), EUNSUPPORTED, "resolution 1 ")
        for start, first, word in ((case["start"] + 1, case["first"], "scaffold 0"), (case["start"], case["first"] + 1, "piece 0"),
                                   (np.where(case["start"] == 11999, 12000, case["start"]), case["first"], "scaffold 3")):
            refused(lambda: _lib.split_maps(missing, case["names"], case["sizes"], first, start, [1000, 2500], [a, b], into=into),
                    EINVAL, word)
        refused(lambda: _split_maps(case, missing, [1000, 2500], [a, b], into=into), EINVAL, "cannot open")
        refused(lambda: _split_maps(case, bad, [1000, 2500], [a, a], into=into), EINVAL, "one context per resolution")
        unchanged()
        # the good file afterwards
        good = _write(tmp_path, case["data"])
        assert _split_maps(case, good, [1000, 2500], [a, b], into=into)[1] is into and into.tobytes() == case["counters"].tobytes()
        assert a.contacts_host().tobytes() == case["maps"][0].tobytes() and b.contacts_host().tobytes() == case["maps"][1].tobytes()


def test_the_pieces_lifted_back_onto_their_parents_give_the_parent_map(tmp_path, monkeypatch):
    """hicmi_lift_maps over the rewritten pairs - pieces as scaffolds, parents as sequences, off = piece_start, nothing
    reversed - is hicmi_build_maps over the original file."""
    from hic_genome_assembler_amd import _lib
    case = _file_case()
    _set_form(monkeypatch, "default")
    path = _write(tmp_path, case["data"])
    rewritten = str(tmp_path / "split.allValidPairs")
    _lib.split_valid_pairs(path, rewritten, case["names"], case["sizes"], case["first"], case["start"], case["piece_names"])
    ctxs = [_lib.Context(0) for _k in range(2 * len(RESOLUTIONS))]
    try:
        parents, lifted = ctxs[:len(RESOLUTIONS)], ctxs[len(RESOLUTIONS):]
        assert _lib.build_maps(path, case["names"], case["sizes"], RESOLUTIONS, parents)[:4] == case["stats"]
        _stats, (_decay, _cis, _trans, unlifted) = _lib.lift_maps(
            rewritten, case["piece_names"], case["piece_sizes"], case["parent"], case["start"], np.zeros(len(case["start"]), np.uint8),
            case["sizes"], RESOLUTIONS, lifted)
        assert int(unlifted[0]) == 0
        for r, p, q in zip(RESOLUTIONS, parents, lifted):
            assert p.contacts_host().tobytes() == q.contacts_host().tobytes() == bref.build(case["pairs"], case["sizes"], r).tobytes()
    finally:
        for ctx in ctxs:
            ctx.close()


# ---- the command line, end to end -----------------------------------------------------------------------------------------------------
def test_cli_end_to_end_through_support_spans_and_parts_1_and_2(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import hostio, splitScaffolds, supportSpans, synth
    from hic_genome_assembler_amd import run_hicAssembler as drv
    _set_form(monkeypatch, "default")
    monkeypatch.setenv("HICMI_LOUVAIN_SEED", "0")
    monkeypatch.setenv("HICMI_NO_PLOTS", "1")
    lay = synth.make_layout(160)
    counts, lay = synth.make_raw_counts(lay)
    r = lay.resolution
    work = str(tmp_path)
    paths = synth.write_hicpro(os.path.join(work, "in"), lay, None)
    pair_file = os.path.join(work, "in", "synth.allValidPairs")
    n_pairs = synth.write_valid_pairs(pair_file, lay, counts)
    names, sizes = hostio.read_scaffold_sizes(paths["hicProScaffSizeFile"])
    # the three longest scaffolds are cut, off the bin grid, the longest one twice; every scaffold is a chromosome of its own,
    # so the junctions of the new order file are the cuts and nothing else
    longest = np.argsort(-sizes, kind="stable")[:3].tolist()
    assert sizes[longest[0]] >= 6 * r and sizes[longest[2]] >= 4 * r
    cuts = {longest[0]: [2 * r + 12345, 4 * r + 7], longest[1]: [2 * r + 1], longest[2]: [2 * r - 1]}
    order = os.path.join(work, "own.orders.txt")
    with open(order, "w") as fh:
        fh.write("".join("### Chromosome grouping %d ###\n%s\t%s\n" % (k + 1, nm, "+-"[k % 2]) for k, nm in enumerate(names)))
    cuts_file = os.path.join(work, "cuts.tsv")
    with open(cuts_file, "w") as fh:
        fh.write("".join("%s\t%d\t0.05\n" % (names[s], c) for s, cs in cuts.items() for c in cs))
    cfg = synth.write_config(os.path.join(work, "config.txt"), paths, os.path.join(work, "out"), os.path.join(work, "plots"), 5 * r,
                             extra={"validPairFile": pair_file})
    out = os.path.join(work, "split")
    splitScaffolds.main(["-config", cfg, "-cuts", cuts_file, "-resolution", str(r), "-order", order, "-out", out, "-threads", "3"])
    said = capsys.readouterr().out
    assert "SPLIT: lines %d, pairs used %d, unknown scaffold 0, out of range 0, chunks 1" % (n_pairs, n_pairs) in said
    assert "SPLIT: 4 cut(s) applied to 3 scaffold(s), 0 skipped, %d piece(s)" % (len(names) + 4) in said
    with open(os.path.join(out, "split_summary.tsv")) as fh:
        summary = [ln.split("\t") for ln in fh.read().splitlines()]
    assert summary[0][:2] == ["#lines=%d" % n_pairs, "used=%d" % n_pairs] and float(summary[2][9]) == n_pairs
    rows = {row[0]: row for row in summary[4:]}
    first, start, _size, _parent = ref.make_pieces(sizes, cuts)
    spanning = {}
    for s, cs in cuts.items():
        for k in range(len(cs)):
            left = rows["%s.brk%d" % (names[s], k + 1)]
            assert left[1] == names[s] and int(left[3]) == sorted(cs)[k] and int(left[8]) > 0
            spanning[("%s.brk%d" % (names[s], k + 1), "%s.brk%d" % (names[s], k + 2))] = int(left[8])
        assert rows["%s.brk%d" % (names[s], len(cs) + 1)][8] == "NA"
    assert all(row[8] == "NA" and row[6] == "0" for name, row in rows.items() if ".brk" not in name)
    # supportSpans on the written inputs: every applied cut is a junction, with the summary's depth
    res_cfg = os.path.join(out, "res%d" % r, "config.txt")
    report = os.path.join(work, "spans.txt")
    supportSpans.main(["-config", res_cfg, "-order", os.path.join(out, "own.orders.txt"), "-step", str(r // 2), "-flank", "1", "-out", report])
    with open(report) as fh:
        lines = fh.read().splitlines()
    junctions = [ln.split("\t") for ln in lines[lines.index("### Junctions ###") + 2:lines.index("### Unplaced ###")]]
    assert len(junctions) == 4 and {tuple(sorted(j[1:3])): int(j[3]) for j in junctions} == {tuple(sorted(k)): v for k, v in spanning.items()}
    # -part1 -part2 on the pieces' map
    capsys.readouterr()
    drv.main(["-part1", "-part2", "-config", res_cfg])
    v = drv.readConfigFileToVariables(res_cfg)
    assert v["validPairFile"] == os.path.join(out, "split.allValidPairs") and v["hicProScaffSizeFile"] == os.path.join(out, "split.sizes")
    for key in ("chromosomeGroupFile", "chromosomeOrderFile", "dendrogramOrderFile", "binGroupFile", "plotOrderFile"):
        assert os.path.getsize(v[key]) > 0, key
