"""The end-link graph on lifted ends on the device (hicmi_links_lifted, hicmi_links_fetch) against
tests/links_lifted_reference.py, for HICMI_LINKS_PLAIN =1, =0 and unset on every case.  Rows and counters are integers, so
every comparison is exact: there are no tolerances.  The refusal of a table above 2^31 slots needs a store of more than 2^30
pairs and is held on the host instead (the capacity rule in tests/test_links_cpu.py)."""
import ctypes
import functools
import os

import numpy as np
import pytest

import liftmap_reference as liftref
import links_lifted_reference as ref
import links_reference as lref
import pairs_reference as pref
import test_links_cpu as cpu
import test_links_lifted_cpu as cpu2

pytestmark = pytest.mark.gpu
EINVAL, EUNSUPPORTED = -1, -5
# Both count forms give the same rows by design: these tests hold each to the reference but cannot tell which kernel ran; that
# the switch is read per call is checked from the source in tests/test_links_lifted_cpu.py.
FORMS = {"default": {}, "plain": {"HICMI_LINKS_PLAIN": "1"}, "combine": {"HICMI_LINKS_PLAIN": "0"}}
ALL = ["plain", "combine", "default"]


def _constants():
    from hic_genome_assembler_amd import _lib
    return _lib.LINKS_SLICE, _lib.LINKS_SLOTS


SLICE, SLOTS = _constants()


def _set_form(monkeypatch, form, first_pairs=None):
    for key in ("HICMI_LINKS_PLAIN", "HICMI_PAIRS_PLAIN", "HICMI_PAIRS_FIRST_PAIRS", "HICMI_BUILDMAP_CHUNK_PAIRS"):
        monkeypatch.delenv(key, raising=False)
    for key, value in FORMS[form].items():
        monkeypatch.setenv(key, value)
    if first_pairs is not None:
        monkeypatch.setenv("HICMI_PAIRS_FIRST_PAIRS", str(first_pairs))


def _want(pairs, sizes, tables, window):
    kept = pref.keep(pairs)
    if len(kept[0]) == 0:
        return ref.NO_ROWS + (np.zeros(4, np.uint64),)
    return ref.rows(kept, sizes, tables, window)


def _same(got, want, n_kept):
    lo, hi, counts, counters = want
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[0].tolist() == lo.tolist() and got[1].tolist() == hi.tolist()
    assert got[2].dtype == np.uint64 and got[2].shape == counts.shape and got[2].tobytes() == counts.tobytes()
    assert got[3].dtype == np.uint64 and got[3].shape == (4,) and got[3].tolist() == counters.tolist()
    # the invariants: the four counters sum to the pairs kept, the rows to linked plus middle
    assert int(got[3].sum()) == n_kept and int(got[2].sum()) == int(got[3][:2].sum()) and int(got[2][:, :4].sum()) == int(got[3][0])


def _every_form(monkeypatch, sizes, parts, cases, n_kept, forms=ALL, **env):
    """One store per form; every (tables, window, want) of ``cases`` counted on it, held to the reference and to the other forms."""
    from hic_genome_assembler_amd import _lib
    made = []
    for form in forms:
        _set_form(monkeypatch, form, **env)
        with _lib.Context(0) as ctx:
            ctx.pairs_begin(sizes)
            for p in parts:
                ctx.pairs_add(*p)
            made.append([ctx.links_lifted(sizes, *tables, window) for tables, window, _want_ in cases])
            ctx.pairs_drop()
        for got, (_tables, _window, want) in zip(made[-1], cases):
            _same(got, want, n_kept)
    for other in made[1:]:
        for a, b in zip(made[0], other):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))                  # the forms with each other
    return made[0]


@functools.lru_cache(maxsize=None)
def _planted_cases():
    P, kept, _sequences, tables = cpu2.planted_round2_tables()
    truth = ref.tables_of(P["true_chroms"], P["sizes"], 100)
    ident = liftref.identity(P["sizes"])
    cases = [(t, 5000, ref.rows(kept, P["sizes"], t, 5000)) for t in (tables, truth, ident)]
    return P, cases


def test_planted_pairs_on_the_paths_of_round_2_on_the_true_chromosomes_and_on_identity_tables(monkeypatch):
    from hic_genome_assembler_amd import _lib
    P, cases = _planted_cases()
    # what the reference gives on the eight paths; on the three chromosomes the zones of 5,000 bases hold few pairs
    assert len(cases[0][0][3]) == 8 and len(cases[0][2][0]) == 28 and cases[0][2][3].tolist() == [240, 4908, 12186, 0]
    assert len(cases[1][0][3]) == 3 and int(cases[1][2][3][2]) > 15000 and len(cases[1][2][0]) == 3
    _every_form(monkeypatch, P["sizes"], [P["pairs"]], cases, 17334)
    # identity tables: the bytes of links_resident on the same store
    _set_form(monkeypatch, "default")
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(P["sizes"])
        ctx.pairs_add(*P["pairs"])
        flat = ctx.links_resident(P["sizes"], 5000)
        lifted = ctx.links_lifted(P["sizes"], *cases[2][0], 5000)
        ctx.pairs_drop()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(flat[:3], lifted[:3]))
    assert lifted[3].tolist() == flat[3].tolist() + [0, 0]


@pytest.mark.parametrize("gap", cpu2.GAPS)
def test_zone_edges(gap, monkeypatch):
    cases, pairs = [], None
    for window in cpu2.WINDOWS:
        sizes, tables, these = cpu2.zone_case(window, gap)
        pairs = these if pairs is None else pairs
        cases.append((tables, window, _want(pairs, sizes, tables, window)))
    _every_form(monkeypatch, cpu.ZONE_SIZES, [pairs], cases, 2000)


@functools.lru_cache(maxsize=None)
def _slice_pool():
    sizes = np.arange(50, 50 + 23, dtype=np.int64)
    tables = ref.tables_of(cpu2.random_sequences(23, 4, drop=0.1), sizes, 100)
    return sizes, tables, cpu.random_pairs(sizes, SLICE + 1, 5)


@pytest.mark.parametrize("n", [SLICE - 1, SLICE, SLICE + 1, 255, 256, 257, 1])
def test_slice_and_workgroup_edges(n, monkeypatch):
    sizes, tables, pool = _slice_pool()
    pairs = tuple(a[:n] for a in pool)
    want = _want(pairs, sizes, tables, 7)
    if n > 255:
        assert all(int(c) > 0 for c in want[3])                                       # every kind of pair takes part
    _every_form(monkeypatch, sizes, [pairs], [(tables, 7, want)], n)


def test_one_key_more_pairs_than_two_slices(monkeypatch):
    # every pair on the key (sequence 0, sequence 1, RL): base 1 of scaffold 3, reversed at the end of sequence 0, with base 10
    # of scaffold 1 at the start of sequence 1
    n = 2 * SLICE + 37
    sizes = np.array([10, 10, 10, 10], dtype=np.int64)
    tables = ref.tables_of([[(0, "+"), (3, "-")], [(1, "-"), (2, "+")]], sizes, 1)
    pairs = (np.full(n, 1, np.int32), np.full(n, 10, np.int64), np.full(n, 3, np.int32), np.ones(n, np.int64))
    want = _want(pairs, sizes, tables, 2)
    assert want[0].tolist() == [0] and want[1].tolist() == [1] and want[2].tolist() == [[0, 0, n, 0, 0]] and want[3].tolist() == [n, 0, 0, 0]
    _every_form(monkeypatch, sizes, [pairs], [(tables, 2, want)], n)


def test_all_keys_distinct_at_the_half_full_bound(monkeypatch):
    # 59 one-scaffold sequences, every second one reversed and their order a permutation of the scaffolds': 8,192 of their 8,555
    # keys, one pair each - four times the slots of the table in LDS, so adds spill, and the global table is exactly half full
    from hic_genome_assembler_amd import _lib
    n = 4 * SLOTS
    S = 59
    assert n <= 5 * S * (S - 1) // 2 and _lib.links_capacity(n, S) == 2 * n
    sizes = np.full(S, 10, dtype=np.int64)
    order = np.random.default_rng(8).permutation(S)
    tables = ref.tables_of([[(int(s), "-" if k % 2 else "+")] for k, s in enumerate(order)], sizes, 100)
    lo, hi = np.triu_indices(S, 1)
    lo, hi, combo = np.repeat(lo, 5), np.repeat(hi, 5), np.tile(np.arange(5), len(lo))
    keep = np.random.default_rng(3).permutation(len(lo))[:n]
    lo, hi, combo = lo[keep], hi[keep], combo[keep]
    # window 2: base 1 is left on a + scaffold and right on a reversed one, base 5 in the middle; the pairs are scattered over
    # the scaffolds, so what the sequences see is left to the reference
    p_lo = np.where(combo == lref.OTHER, 5, np.where(combo // 2 == 0, 1, 10))
    p_hi = np.where(combo == lref.OTHER, 1, np.where(combo % 2 == 0, 1, 10))
    pairs = (hi.astype(np.int32), p_hi.astype(np.int64), lo.astype(np.int32), p_lo.astype(np.int64))
    want = _want(pairs, sizes, tables, 2)
    assert int((want[2] > 0).sum()) == n and int(want[2].max()) == 1 and want[3].tolist()[2:] == [0, 0]
    _every_form(monkeypatch, sizes, [pairs], [(tables, 2, want)], n)


def test_one_sequence_every_scaffold_dropped_and_an_empty_store(monkeypatch):
    sizes = cpu.ZONE_SIZES
    pairs = cpu.random_pairs(sizes, 700, 3)
    one = ref.tables_of([[(s, "-" if s % 2 else "+") for s in range(len(sizes))]], sizes, 1)
    dropped = (np.full(len(sizes), -1, np.int32), one[1], one[2], one[3])
    none = ref.NO_ROWS
    cases = [(one, 5, none + (np.asarray([0, 0, 700, 0], np.uint64),)), (dropped, 5, none + (np.asarray([0, 0, 0, 700], np.uint64),))]
    assert all(all(a.tobytes() == b.tobytes() for a, b in zip(_want(pairs, sizes, t, w), want)) for t, w, want in cases)
    _every_form(monkeypatch, sizes, [pairs], cases, 700)
    empty = none + (np.zeros(4, np.uint64),)
    for parts in ([], [cpu._pairs([])], [cpu._pairs([(1, 2, 1, 1)] * 5)]):
        _every_form(monkeypatch, sizes, parts, [(one, 5, empty), (liftref.identity(sizes), 5, empty)], 0)


def test_a_grown_store_a_reordered_store_and_either_store_order(monkeypatch):
    from hic_genome_assembler_amd import _lib
    sizes, tables, pairs = cpu2.zone_case(5, 100)
    want = _want(pairs, sizes, tables, 5)
    parts = [tuple(a[k:k + 300] for a in pairs) for k in range(0, 2000, 300)]
    _every_form(monkeypatch, sizes, parts, [(tables, 5, want)], 2000, first_pairs=256)          # several growths
    sa, pa, sb, pb = pairs
    order = np.random.default_rng(9).permutation(2000)
    _every_form(monkeypatch, sizes, [(sb[order], pb[order], sa[order], pa[order])], [(tables, 5, want)], 2000)
    for store in ("0", "1"):
        _set_form(monkeypatch, "combine")
        monkeypatch.setenv("HICMI_PAIRS_PLAIN", store)
        with _lib.Context(0) as ctx:
            ctx.pairs_begin(sizes)
            ctx.pairs_add(*pairs)
            _same(ctx.links_lifted(sizes, *tables, 5), want, 2000)
            ctx.pairs_drop()


def _fetch(ctx, n_rows):
    from hic_genome_assembler_amd import _lib
    lo, hi, counts = np.zeros(n_rows, np.int32), np.zeros(n_rows, np.int32), np.zeros((n_rows, 5), np.uint64)
    assert ctx._lib.hicmi_links_fetch(ctx._h, _lib._ptr(lo), _lib._ptr(hi), _lib._ptr(counts)) == 0
    return lo, hi, counts


def test_the_rows_of_a_lifted_call_replace_those_of_a_scaffold_call_and_the_other_way_round(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    sizes, tables, pairs = cpu2.zone_case(5, 1)
    want, flat = _want(pairs, sizes, tables, 5), lref.rows(pref.keep(pairs), sizes, 5)
    assert len(want[0]) != len(flat[0])
    with _lib.Context(0) as ctx:
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        got = ctx.links_resident(sizes, 5)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, flat))
        _same(ctx.links_lifted(sizes, *tables, 5), want, 2000)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_fetch(ctx, len(want[0])), want[:3]))      # the lifted rows are the context's
        records, slots, _ms = ctx.links_info()
        assert records == int((want[2] > 0).sum()) and slots == _lib.links_capacity(2000, len(tables[3]))
        got = ctx.links_resident(sizes, 5)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, flat))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_fetch(ctx, len(flat[0])), flat[:3]))
        _same(ctx.links_lifted(sizes, *tables, 5), want, 2000)
        ctx.pairs_add(*(a[:10] for a in pairs))                                          # pairs added afterwards make the rows stale
        assert ctx._lib.hicmi_links_fetch(ctx._h, None, None, None) == EINVAL
        twice = tuple(np.concatenate([a, a[:10]]) for a in pairs)
        _same(ctx.links_lifted(sizes, *tables, 5), _want(twice, sizes, tables, 5), 2010)
        ctx.pairs_drop()
        assert ctx._lib.hicmi_links_fetch(ctx._h, None, None, None) == EINVAL


# ---- refusals: every one leaves marked output buffers untouched -------------------------------------------------------------------------
def _raw(ctx, sizes, tables, window, n_scaf=None, n_seq=None, null=None):
    from hic_genome_assembler_amd import _lib
    size, seq, off, rev, seq_size = _lib._lift_tables(sizes, *tables)
    counters = np.full(4, 0xABAB, np.uint64)
    n_rows = ctypes.c_int64(-7)
    args = [_lib._ptr(size), len(size) if n_scaf is None else n_scaf, _lib._ptr(seq), _lib._ptr(off), _lib._ptr(rev), _lib._ptr(seq_size),
            len(seq_size) if n_seq is None else n_seq, int(window), ctypes.byref(n_rows), _lib._ptr(counters)]
    if null is not None:
        args[null] = None
    rc = ctx._lib.hicmi_links_lifted(ctx._h, *args)
    return rc, n_rows.value, counters.tolist(), _lib.load().hicmi_last_error().decode("utf-8", "replace")


def _unwritten(got):
    return got[1] == -7 and got[2] == [0xABAB] * 4


def test_refusals_leave_the_outputs_and_the_rows_as_they_were(monkeypatch):
    from hic_genome_assembler_amd import _lib
    _set_form(monkeypatch, "default")
    sizes, tables, pairs = cpu2.zone_case(5, 100)
    pairs = tuple(a[:500] for a in pairs)
    want = _want(pairs, sizes, tables, 5)
    seq, off, rev, seq_sizes = tables

    def changed(k, at, value):
        out = [np.array(t) for t in tables]
        out[k][at] = value
        return tuple(out)

    first = int(np.argmax(off > 0))                                                   # a scaffold behind another one in its sequence
    with _lib.Context(0) as ctx:
        got = _raw(ctx, sizes, tables, 5)
        assert got[0] == EINVAL and "hicmi_links_lifted without a pair store" in got[3] and _unwritten(got)
        ctx.pairs_begin(sizes)
        ctx.pairs_add(*pairs)
        other = sizes.copy()
        other[3] += 1
        refusals = [(dict(sizes=other), EINVAL, "sizes"), (dict(sizes=sizes[:-1], tables=tuple(t[:-1] for t in tables[:3]) + (seq_sizes,)), EINVAL, "sizes"),
                    (dict(window=0), EINVAL, "window 0 is below 1"), (dict(window=-5), EINVAL, "window"),
                    (dict(tables=changed(0, 2, len(seq_sizes))), EINVAL, "lies in sequence"), (dict(tables=changed(0, 2, -2)), EINVAL, "lies in sequence"),
                    (dict(tables=changed(1, 2, -1)), EINVAL, "negative offset"), (dict(tables=changed(1, first, 0)), EINVAL, "overlap"),
                    (dict(tables=changed(3, int(seq[first]), int(seq_sizes[seq[first]]) - 1)), EINVAL, "ends beyond"),
                    (dict(tables=changed(3, 0, -1)), EINVAL, "negative size"), (dict(n_seq=0), EINVAL, "bad arguments")]
        refusals += [(dict(null=k), EINVAL, "bad arguments" if k else "sizes") for k in (0, 2, 3, 4, 5, 8, 9)]
        for rows_before in (False, True):
            if rows_before:                                                           # a count, then the refusals: its rows stay
                _same(ctx.links_lifted(sizes, *tables, 5), want, 500)
            for kw, code, word in refusals:
                args = dict(sizes=sizes, tables=tables, window=5)
                args.update(kw)
                got = _raw(ctx, args.pop("sizes"), args.pop("tables"), args.pop("window"), **args)
                assert got[0] == code and word in got[3] and _unwritten(got), (kw, got)
            if rows_before:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(_fetch(ctx, len(want[0])), want[:3]))
            else:
                assert ctx._lib.hicmi_links_fetch(ctx._h, None, None, None) == EINVAL    # a store, but no count yet
        ctx.pairs_drop()
        with pytest.raises(_lib.HicmiError) as exc:
            ctx.links_lifted(sizes, *tables, 5)
        assert "error %d:" % EINVAL in str(exc.value) and "without a pair store" in str(exc.value)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_cli_rounds_on_the_planted_pair_file_and_placeunplaced_on_the_final_order(tmp_path, monkeypatch, capsys):
    from hic_genome_assembler_amd import placeUnplaced, scaffoldLinks
    _set_form(monkeypatch, "default")
    P, cfg, order, _save = cpu.planted_files(tmp_path)
    made = {}
    for where, context in (("device", None), ("stand_in", ref.StandInContext())):
        out = str(tmp_path / where)
        _stats, joins, paths = scaffoldLinks.main(["-config", cfg, "-window", "5000", "-rounds", "5", "-order", order, "-out", out,
                                                   "-threads", "3"], context=context)
        assert len(joins) == 32 and len(paths) == 8
        made[where] = {os.path.relpath(os.path.join(d, fn), out): cpu._read(os.path.join(d, fn)) for d, _sub, fns in os.walk(out) for fn in fns}
    assert made["device"] == made["stand_in"] and len(made["device"]) == 5 + 2 + 2 * 4
    assert capsys.readouterr().out.count("LINKS: 3 rounds, ended nothing_left, paths 3, singles 0\n") == 2
    final = os.path.join(str(tmp_path / "device"), "final.order")
    cpu2.check_final_order(final, P)
    # the final layout is an order file placeUnplaced runs on: every scaffold lies in a path, so it has nothing to place
    report = str(tmp_path / "unplaced.txt")
    placeUnplaced.main(["-config", cfg, "-order", final, "-window", "5000", "-out", report])
    assert os.path.isfile(report)
