"""Inversion support and the refinement on the GPU (k_part2_invert.hip through hicmi_p2_inversions_multi;
orderGenome.refineOrdering) against the CPU oracle's literal cost of every candidate's explicit bin order and the
restated greedy loop (tests/inversion_reference.py).

Tolerances (fixed before any run, those of tests/test_gpu_support.py): a score within 1e-10 relative of the oracle's; a
delta is the difference of two such scores: 2e-10 * |score0| absolute; the best right end EQUAL to the oracle's first
strict maximum.  A verdict is compared wherever the oracle's |best_delta| is larger than that absolute bound (below it
the sign of a difference of two fp64 scores is not defined); for n160, n600 and n2000 no such row may exist."""
import contextlib
import io
import os

import numpy as np
import pytest

import golden_cases as gc
import inversion_reference as ref
from support_reference import read_group_file, read_order_file, write_order_file

pytestmark = pytest.mark.gpu

REL = 1e-10
GOLDEN = [n for n in gc.case_names() if os.path.exists(os.path.join(gc.GOLDEN_DIR, n, "chromosomeOrders.txt"))]
NO_INVERTIBLE = ("n160", "n600", "n2000")     # checked on the CPU: no row of these golden orders is invertible
REFINE_CASES = [("n600", 0), ("n2000", 0), ("n2000", 5)]


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    monkeypatch.delenv("HICMI_P2_INVERT_DIRECT", raising=False)
    monkeypatch.delenv("HICMI_P2_INVERT_MAX_WORK", raising=False)


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _inputs(name, tmp_path):
    paths = _quiet(gc.write_case_files, name, str(tmp_path))
    files = {fn: os.path.join(gc.GOLDEN_DIR, name, fn) for fn in ("chromosomeGroups.txt", "chromosomeOrders.txt")}
    return paths, files["chromosomeGroups.txt"], files["chromosomeOrders.txt"]


def _inversions(paths, groups, orders, out, **kw):
    from hic_genome_assembler_amd import supportInversions as si
    return _quiet(si.runInversions, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups, orders,
                  out, **kw)


def _compare(results, expected, label, max_span=0):
    """The whole tables, score0, the best right ends, their deltas and the verdicts against the oracle; prints the figures
    before asserting them.  Returns the smallest |gain| of a row with a best inversion."""
    worst, worst_delta, margin, gain = 0.0, 0.0, np.inf, np.inf
    problems = []
    for k, (got, exp) in enumerate(zip(results, expected)):
        assert got["names"] == exp["names"] and got["orientations"] == exp["orientations"]
        s0, S = exp["score0"], len(exp["names"])
        t_got, t_exp = np.asarray(got["table"]), exp["table"]
        assert t_got.shape == t_exp.shape == (S, S)
        if s0 != 0.0:
            worst = max(worst, abs(got["total"] - exp["total"]) / abs(exp["total"]), abs(got["score0"] - s0) / abs(s0))
            scored = t_exp != 0.0
            assert not t_got[~scored].any()                   # left of the diagonal and beyond max_span: 0.0
            if scored.any():
                worst = max(worst, float(np.max(np.abs(t_got[scored] - t_exp[scored]) / np.abs(t_exp[scored]))))
        else:
            assert got["score0"] == 0.0 and got["total"] == exp["total"] and not t_got.any()
        bound = 2 * REL * abs(s0)
        for i, e in exp["rows"].items():
            g = got["rows"][i]
            if g["bins"] != e["bins"]:
                problems.append((k, i, "bins", g["bins"], e["bins"]))
            if e["best"] is None:
                if not (g["best_j"] is None and g["best_end"] is None and g["span"] is None and g["span_bins"] is None
                        and g["best_delta"] is None and g["gain"] is None and g["verdict"] == "NA"):
                    problems.append((k, i, "best", g["best_j"], None))
                continue
            margin, gain = min(margin, e["margin"] / abs(s0)), min(gain, abs(e["gain"]))
            if (g["best_j"], g["best_end"], g["span"], g["span_bins"]) != (e["best"], e["end"], e["span"], e["span_bins"]):
                problems.append((k, i, "best", (g["best_j"], g["best_end"], g["span"], g["span_bins"]),
                                 (e["best"], e["end"], e["span"], e["span_bins"])))
                continue
            worst_delta = max(worst_delta, abs(g["best_delta"] - e["delta"]) / abs(s0))
            if abs(e["delta"]) > bound and g["verdict"] != e["verdict"]:
                problems.append((k, i, "verdict", g["verdict"], e["verdict"]))
    print("%s: largest relative error of a score %.3e (bound %.0e), of a delta / score0 %.3e (bound %.0e), smallest |gain| "
          "%.3e, smallest relative margin of a best inversion over its runner-up or score0 %.3e"
          % (label, worst, REL, worst_delta, 2 * REL, gain, margin))
    assert not problems, problems[:10]
    assert worst <= REL
    assert worst_delta <= 2 * REL
    return gain


def _shape(text):
    """A report without its floats: header prefixes, and per scaffold everything but best_delta and gain."""
    return [ln.split(" ### ")[0] if ln.startswith("#") else ln.split("\t")[:6] + ln.split("\t")[8:] for ln in text.splitlines()]


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_orders_against_the_oracle(name, tmp_path):
    paths, groups, orders = _inputs(name, tmp_path)
    results = _inversions(paths, groups, orders, str(tmp_path / "inv.txt"), fullDir=str(tmp_path / "full"))
    expected = _quiet(ref.reference_for_files, paths, groups, orders)
    rows = [r for x in expected for r in x["rows"].values()]
    counts = {v: sum(r["verdict"] == v for r in rows) for v in ("invertible", "supported", "NA")}
    print(name, "rows by the oracle's verdict:", counts)
    gain = _compare(results, expected, name)
    got_rows = [r for x in results for r in x["rows"]]
    if name in NO_INVERTIBLE:
        assert counts["invertible"] == 0
        assert gain > 1e-9                                    # the smallest |best_delta| is far outside the tie band
        for verdict in counts:
            assert sum(r["verdict"] == verdict for r in got_rows) == counts[verdict]
    else:                                                     # the other goldens: whatever the oracle finds
        undecided = sum(r["best"] is not None and abs(r["gain"]) <= 2 * REL for r in rows)
        print(name, "rows whose |gain| is inside the bound of a delta (verdict not compared):", undecided)
        if undecided == 0:
            for verdict in counts:
                assert sum(r["verdict"] == verdict for r in got_rows) == counts[verdict]
    with open(str(tmp_path / "inv.txt")) as fh:
        report = fh.read()
    assert _shape(report) == _shape(ref.report_text(expected))
    with open(str(tmp_path / "full" / "Chr_1.inversions.tsv")) as fh:
        full = fh.read().splitlines()
    assert full[0] == ref.full_text(expected[0]).splitlines()[0] and len(full) == len(expected[0]["names"]) + 1


@pytest.mark.parametrize("name", ["n600", "n2000"])
def test_planted_inversions_are_found_and_undone(name, tmp_path):
    from hic_genome_assembler_amd import orderGenome as p2
    paths, groups, orders = _inputs(name, tmp_path)
    golden = read_order_file(orders)
    planted, blocks = ref.plant_inversions(golden)
    assert len(blocks) == {"n600": 5, "n2000": 9}[name]
    orders2 = str(tmp_path / "planted.txt")
    write_order_file(orders2, planted)
    results = _inversions(paths, groups, orders2, str(tmp_path / "inv.txt"))
    expected = _quiet(ref.reference_for_files, paths, groups, orders2)
    _compare(results, expected, name + " with planted inversions")
    host, where = _quiet(ref.host_and_where, paths, groups)
    rows_of = read_group_file(groups)
    for k, (i, j) in blocks.items():
        row, want = results[k]["rows"][i], expected[k]["rows"][i]
        gold = ref.literal_score(host, where, rows_of[k], golden[k])
        print(name, "chromosome %d: planted %d..%d, best_end %s, gain %.3e, margin %.3e" % (k + 1, i, j, row["best_j"], row["gain"],
                                                                                            want["margin"]))
        assert want["verdict"] == "invertible" and want["best"] == j and want["margin"] >= 1.4e-2
        assert row["verdict"] == "invertible" and row["best_j"] == j and row["best_end"] == planted[k][j][0]
        # applying it gives the golden arrangement and its score
        ids, rev = p2.apply_move(range(len(planted[k])), [o == "-" for _n, o in planted[k]], ("invert", i, j, row["best_delta"]))
        assert [(planted[k][a][0], "-" if r else "+") for a, r in zip(ids, rev)] == golden[k]
        assert abs(results[k]["score0"] + row["best_delta"] - gold) <= 2 * REL * abs(gold)
        assert expected[k]["table"][i, j] == gold


def _decay_block(n, seed):
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    c = rng.uniform(0.5, 1.5, (n, n)) * 100.0 / (1.0 + np.abs(idx[:, None] - idx[None, :])) ** 1.1
    return np.triu(c) + np.triu(c, 1).T


def _chromosome(prefix, first, lens):
    out, pos = [], first
    for i, ln in enumerate(lens):
        out.append(("%s%d" % (prefix, i), range(pos, pos + ln)))
        pos += ln
    return out, pos


def _build(spec, seed, ones=False):
    """Chromosomes [(prefix, scaffold lengths)] side by side in one matrix whose contacts lie inside the chromosomes (no
    call reads any other cell): a decaying block each, arrangements shuffled and half of the scaffolds '-'."""
    rng = np.random.default_rng(seed)
    groups, arrs, pos = [], [], 0
    for prefix, lens in spec:
        g, pos = _chromosome(prefix, pos, lens)
        groups.append(g)
        order = rng.permutation(len(lens))
        arrs.append([(g[i][0], "-" if rng.random() < 0.5 else "+") for i in order])
    host = np.zeros((pos, pos))
    for k, g in enumerate(groups):
        a, b = g[0][1][0], g[-1][1][-1] + 1
        host[a:b, a:b] = 1.0 if ones else _decay_block(b - a, seed + k)
    return host, groups, arrs


def _explicit(host, groups, arrangements):
    from hic_genome_assembler_amd import orderGenome as p2
    from hic_genome_assembler_amd.hostio import Bin
    binList = [Bin(1000 + i, "c", i, i + 1, 1.0, 0.0) for i in range(len(host))]
    chromList = [sorted([binList[i].ID, name] for name, idx in g for i in idx) for g in groups]
    ordered = []
    for rows, arr in zip(chromList, arrangements):
        bins_of = {}
        for b, x in rows:
            bins_of.setdefault(x, []).append(b)
        scaffs = []
        for name, o in arr:
            s = p2.Scaffold(name, sorted(bins_of[name]), "+")
            if o == "-":
                s.flipOrientation()
            scaffs.append(s)
        ordered.append(scaffs)
    return binList, chromList, ordered


def _run_explicit(host, groups, arrangements, max_span=0, oracle=True):
    """inversionSupport on chromosomes given as [(scaffold, row indices)] lists and [(scaffold, orientation)]
    arrangements, and the oracle on the same."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    binList, chromList, ordered = _explicit(host, groups, arrangements)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(host)
        results = p2.inversionSupport(p2.GenomeMatrix(ctx), ordered, binList, chromList, maxSpan=max_span)
    where = {b.ID: i for i, b in enumerate(binList)}
    expected = [ref.oracle_inversions(host, where, rows, arr, max_span)
                for rows, arr in zip(chromList, arrangements)] if oracle else None
    return results, expected


SMALL = (("one", [9]), ("two", [3, 4]), ("three", [2, 1, 5]), ("dots", [1] * 7), ("bin", [1]), ("dark", [3, 2, 2, 1]),
         ("w63", [63, 200, 55]), ("w64", [64, 200, 56]), ("w65", [65, 200, 57]), ("mix", [7, 1, 6, 2, 1, 12, 3]))


@pytest.fixture(scope="module")
def small():
    """S = 1, 2 and 3; one-bin scaffolds only; one bin; no contacts; segments of 63, 64 and 65 bins beside outsides of 255,
    256 and 257 positions (and the reverse); a mixed chromosome of 7 scaffolds."""
    host, groups, arrs = _build(SMALL, 5)
    dark = [i for _name, idx in groups[5] for i in idx]
    host[np.ix_(dark, dark)] = 0.0                            # its total is 0: nothing to score
    return host, groups, arrs


def test_edge_shapes_in_one_call(small):
    """The small shapes, S = 258 one-bin scaffolds (the pick's second 256-lane trip), 1,100 bins beside 20 and 8,300 bins
    in 6 scaffolds beside 90 bins, all in ONE hicmi_p2_inversions_multi call."""
    from hic_genome_assembler_amd import orderGenome as p2
    spec = SMALL + (("trip", [1] * 258), ("big", [1100, 100, 60, 37, 1, 2]), ("small", [7, 5, 1, 4, 3]),
                    ("huge", [4000, 2500, 1200, 500, 90, 10]), ("beside", [40, 30, 15, 5]))
    host, groups, arrs = _build(spec, 5)
    dark = [i for _name, idx in groups[5] for i in idx]
    host[np.ix_(dark, dark)] = 0.0
    results, expected = _run_explicit(host, groups, arrs)
    by = {p: k for k, (p, _l) in enumerate(spec)}
    assert expected[by["huge"]]["n"] == 8300 and expected[by["beside"]]["n"] == 90 and expected[by["big"]]["n"] == 1300
    _compare(results, expected, "edge shapes")
    for name in ("one", "two", "bin", "dark"):
        assert [r["verdict"] for r in results[by[name]]["rows"]] == ["NA"] * len(results[by[name]]["rows"]), name
    assert results[by["bin"]]["score0"] == 0.0 and results[by["dark"]]["total"] == 0.0
    assert not results[by["dark"]]["table"].any() and not results[by["bin"]]["table"].any()
    three = results[by["three"]]["rows"]
    assert [r["best_j"] for r in three] == [1, 2, None]       # S = 3: (0, 1) and (1, 2) compete, (0, 2) is the mirror image
    trip = results[by["trip"]]
    assert trip["table"].shape == (258, 258) and trip["rows"][0]["best_j"] is not None and trip["rows"][257]["verdict"] == "NA"
    assert max(r["best_j"] or 0 for r in trip["rows"]) > 0
    assert p2.inversionSupportText(results).count("\tNA\tNA\tNA\tNA\tNA\tNA\n") == \
        sum(r["best"] is None for x in expected for r in x["rows"].values())
    assert _shape(p2.inversionSupportText(results)) == _shape(ref.report_text(expected))


def test_the_diagonal_is_placement_supports_flip_in_place(small):
    """Two kernels, one number: table[i][i] against hicmi_p2_support's score of scaffold i at its own gap in the other
    orientation, on the same arrangements, within 1e-10."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    host, groups, arrs = small
    binList, chromList, ordered = _explicit(host, groups, arrs)
    worst, seen = 0.0, 0
    with _lib.Context(0) as ctx:
        ctx.set_contacts(host)
        matrix = p2.GenomeMatrix(ctx)
        matrix.bin_index(binList)
        (jobs,) = p2._layout_jobs(matrix.lanes(len(ordered)), ordered, binList, chromList)
        sup = _lib.Context.p2_support_multi([(layout.ctx, ids, rev, total) for layout, ids, rev, total, _g in jobs])
        inv = _lib.Context.p2_inversions_multi([(layout.ctx, ids, rev, total) for layout, ids, rev, total, _g in jobs])
        for (layout, ids, rev, total, _g), (st, _sb), (it, _ib) in zip(jobs, sup, inv):
            if layout.n < 2 or not total > 0:
                assert not it.any()
                continue
            for i in range(len(ids)):
                want = st[i, i, 1 - int(rev[i])]
                worst = max(worst, abs(it[i, i] - want) / abs(want))
                seen += 1
    print("diagonal against hicmi_p2_support: %d scaffolds, largest relative difference %.3e" % (seen, worst))
    assert seen == 29 and worst <= REL                        # every scaffold of the eight chromosomes with contacts


@pytest.mark.parametrize("max_span", [2, 3])
def test_max_span_zeroes_the_table_beyond_and_narrows_the_picks(small, max_span):
    host, groups, arrs = small
    full, _e = _run_explicit(host, groups, arrs, oracle=False)
    cut, expected = _run_explicit(host, groups, arrs, max_span=max_span)
    _compare(cut, expected, "small shapes, maxSpan %d" % max_span, max_span)
    narrowed = 0
    for a, b in zip(full, cut):
        S = len(a["names"])
        i, j = np.indices((S, S))
        inside = (j >= i) & (j - i + 1 <= max_span)
        assert np.array_equal(np.asarray(a["table"])[inside], np.asarray(b["table"])[inside])   # the same bits inside the span
        assert not np.asarray(b["table"])[~inside].any() and a["score0"] == b["score0"]
        for ra, rb in zip(a["rows"], b["rows"]):
            assert rb["span"] is None or 2 <= rb["span"] <= max_span
            narrowed += ra["best_j"] != rb["best_j"]
    print("maxSpan %d against 0: best ends that moved: %d" % (max_span, narrowed))
    assert narrowed > 0


@pytest.mark.parametrize("kind", ["decay", "ones"])
def test_best_is_the_summary_of_the_devices_own_table(kind):
    """The device's pick against its host restatement on the SAME doubles: ``best`` of hicmi_p2_inversions_multi equals
    inversion_summary of the table that call returned - integer equality, no tolerance.  S = 258 (the pick's second
    256-lane trip), 255 ... 257 around the stride and the exits S = 1, 2, 3; max_span 0 and 3.  On the map of ones many
    scores are exactly equal: the first of equals wins and near counts above 1 must occur."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    spec = (("a", [1] * 258), ("b", [1] * 255), ("c", [2] + [1] * 255), ("d", [1] * 257), ("e", [4]), ("f", [2, 3]),
            ("g", [1, 2, 3]), ("h", [3, 1, 4, 1, 5, 9, 2, 6]))
    host, groups, arrs = _build(spec, 43, ones=kind == "ones")
    binList, chromList, ordered = _explicit(host, groups, arrs)
    near = 0
    with _lib.Context(0) as ctx:
        ctx.set_contacts(host)
        matrix = p2.GenomeMatrix(ctx)
        matrix.bin_index(binList)
        (jobs,) = p2._layout_jobs(matrix.lanes(len(ordered)), ordered, binList, chromList)
        for max_span in (0, 3):
            out = _lib.Context.p2_inversions_multi([(layout.ctx, ids, rev, total) for layout, ids, rev, total, _g in jobs],
                                                   max_span)
            for (layout, ids, _r, _t, _g), (table, best) in zip(jobs, out):
                assert table.shape == (len(ids), len(ids)) and np.isfinite(table).all()
                assert np.array_equal(best, p2.inversion_summary(table, max_span)), (max_span, len(ids))
                near = max(near, int(best[:, 1].max()))
    print(kind, "map: largest near count", near)
    assert near > 1 or kind == "decay"


def test_an_oversized_call_is_refused_before_any_launch(small, monkeypatch):
    """The bound on a call's work is a condition on host arithmetic: with the bound faked down to 1,000 matrix reads the
    small shapes are refused with HICMI_EUNSUPPORTED and a message naming max_span, nothing is launched, and the same call
    runs once the bound is back."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    host, groups, arrs = small
    binList, chromList, ordered = _explicit(host, groups, arrs)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(host)
        matrix = p2.GenomeMatrix(ctx)
        monkeypatch.setenv("HICMI_P2_INVERT_MAX_WORK", "1000")
        with pytest.raises(_lib.HicmiError) as err:
            p2.inversionSupport(matrix, ordered, binList, chromList)
        assert "error -5" in str(err.value) and "max_span" in str(err.value)
        monkeypatch.delenv("HICMI_P2_INVERT_MAX_WORK")
        assert len(p2.inversionSupport(matrix, ordered, binList, chromList)) == len(ordered)
    lengths = [len(idx) for _n, idx in groups[9]]
    assert p2.inversion_work(lengths) > 1000 and p2.inversion_work([10] * 4096) > 1e13


@pytest.mark.parametrize("name", ["n600", "n2000"])
def test_default_path_against_direct(name, tmp_path, monkeypatch):
    paths, groups, orders = _inputs(name, tmp_path)
    a = _inversions(paths, groups, orders, str(tmp_path / "a.txt"), fullDir=str(tmp_path / "full_a"))
    again = _inversions(paths, groups, orders, str(tmp_path / "a2.txt"), fullDir=str(tmp_path / "full_a2"))
    monkeypatch.setenv("HICMI_P2_INVERT_DIRECT", "1")
    b = _inversions(paths, groups, orders, str(tmp_path / "b.txt"))
    worst = 0.0
    for x, y, z in zip(a, b, again):
        assert x["score0"] == y["score0"] and x["total"] == y["total"]
        assert np.array_equal(x["table"], z["table"])                       # a second call gives the same bits
        scored = np.asarray(y["table"]) != 0.0
        assert np.array_equal(scored, np.asarray(x["table"]) != 0.0)
        if scored.any():
            worst = max(worst, float(np.max(np.abs(x["table"][scored] - y["table"][scored]) / np.abs(y["table"][scored]))))
        for r, q in zip(x["rows"], y["rows"]):
            assert (r["best_j"], r["span"], r["verdict"], r["bins"]) == (q["best_j"], q["span"], q["verdict"], q["bins"])
    print(name, "default against DIRECT: largest relative difference of a score %.3e" % worst)
    assert worst <= REL
    texts = []
    for fn in ("a.txt", "b.txt", "a2.txt", os.path.join("full_a", "Chr_1.inversions.tsv"), os.path.join("full_a2", "Chr_1.inversions.tsv")):
        with open(str(tmp_path / fn)) as fh:
            texts.append(fh.read())
    assert texts[0] == texts[1] == texts[2]                   # the reported floats are literal scores on both paths
    assert texts[3] == texts[4] and len(texts[3].splitlines()) > 1


# ---- refinement ---------------------------------------------------------------------------------------
_GREEDY = {}


def _greedy_all(name, paths, groups, orders_list, chrom=None, **kw):
    """The restated greedy loop on every chromosome of an ordering.  The golden start is computed once per case; a start
    that differs from the golden order in chromosome ``chrom`` alone re-uses it for every other chromosome that the golden
    start leaves without a move (no move with both families in round 1: none with fewer families or fewer rounds)."""
    host, where = _quiet(ref.host_and_where, paths, groups)
    rows_of = read_group_file(groups)
    if name not in _GREEDY:
        golden = read_order_file(os.path.join(gc.GOLDEN_DIR, name, "chromosomeOrders.txt"))
        _GREEDY[name] = [ref.greedy(host, where, rows, arr) for rows, arr in zip(rows_of, golden)]
    if chrom is None:
        return _GREEDY[name]
    return [_GREEDY[name][k] if k != chrom and not _GREEDY[name][k][1] else ref.greedy(host, where, rows_of[k], arr, **kw)
            for k, arr in enumerate(orders_list)]


def _refine(paths, groups, orders, out, **kw):
    from hic_genome_assembler_amd import refinePart2 as rp
    return _quiet(rp.runRefine, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups, orders,
                  "plotOrder.txt", out, **kw)


def _check_refinement(got, want, out_dir, order_name):
    """Moves, rounds, convergence and the written files of a run against the restated loop."""
    refined, log, summary = got
    moves = [[e["move"][:-1] for e in log if e["chromosome"] == k + 1] for k in range(len(want))]
    for k, (arr, applied, rounds, converged, before, after) in enumerate(want):
        mine = [(m[0], m[1], m[2], "-" if m[3] else "+") if m[0] == "relocate" else m for m in moves[k]]
        assert mine == applied, (k, mine, applied)
        assert [(s.name, s.orientation) for s in refined[k]] == arr
        assert (summary[k]["moves"], summary[k]["rounds"], summary[k]["converged"]) == (len(applied), rounds, converged)
        assert abs(summary[k]["before"] - before) <= REL * abs(before) and abs(summary[k]["after"] - after) <= 2 * REL * abs(after)
    ref_path = os.path.join(out_dir, "want.txt")
    write_order_file(ref_path, [w[0] for w in want])
    with open(ref_path) as fa, open(os.path.join(out_dir, order_name)) as fb:
        assert fa.read() == fb.read()
    with open(os.path.join(out_dir, "refine.log")) as fh:
        assert len(fh.read().splitlines()) == sum(len(w[1]) for w in want)
    with open(os.path.join(out_dir, "refine_summary.tsv")) as fh:
        lines = fh.read().splitlines()
    assert [ln.split("\t")[3:] for ln in lines[1:]] == [[str(len(w[1])), str(w[2]), "yes" if w[3] else "no"] for w in want]
    with open(os.path.join(out_dir, "plotOrder.txt")) as fh:
        assert fh.readline() == "#ScaffoldID\tHiCPro-BinID\n"


@pytest.mark.parametrize("name,chrom", REFINE_CASES)
def test_refinement_from_the_two_starts(name, chrom, tmp_path):
    """From the planted inversion the climb reaches the golden arrangement in 1 move; from "planted inversion, then
    scaffold 1 moved to gap S - 2 and flipped" in 2, the inversion first; relocations alone do not get there in one move;
    -maxRounds 1 on the two-fault start reports not converged."""
    paths, groups, orders = _inputs(name, tmp_path)
    golden = read_order_file(orders)
    S = len(golden[chrom])
    i, j = ref.planted_block(S)
    one = [list(a) for a in golden]
    one[chrom] = ref.invert_arrangement(golden[chrom], i, j)
    two = [list(a) for a in one]
    two[chrom] = ref.relocate_arrangement(one[chrom], 1, S - 2, "-" if one[chrom][1][1] == "+" else "+")
    host, where = _quiet(ref.host_and_where, paths, groups)
    gold = ref.literal_score(host, where, read_group_file(groups)[chrom], golden[chrom])
    for label, start, n_moves in (("one", one, 1), ("two", two, 2)):
        path, out = str(tmp_path / (label + ".txt")), str(tmp_path / label)
        write_order_file(path, start)
        with open(path) as fh:
            before = fh.read()
        got = _refine(paths, groups, path, out)
        want = _greedy_all(name, paths, groups, start, chrom)
        _check_refinement(got, want, out, label + ".txt")
        kinds = [e["kind"] for e in got[1] if e["chromosome"] == chrom + 1]
        print(name, "chromosome", chrom + 1, label, "fault(s):", [e["move"] for e in got[1] if e["chromosome"] == chrom + 1])
        assert kinds == ["invert", "relocate"][:n_moves]
        assert [(s.name, s.orientation) for s in got[0][chrom]] == golden[chrom] and got[2][chrom]["converged"]
        assert abs(got[2][chrom]["after"] - gold) <= 2 * REL * abs(gold)
        with open(path) as fh:
            assert fh.read() == before                        # the input order file is never changed
    # relocations alone: one move does not reach the golden score
    got = _refine(paths, groups, str(tmp_path / "one.txt"), str(tmp_path / "rel"), moves=("relocate",), maxRounds=1)
    want = _greedy_all(name, paths, groups, one, chrom, moves=("relocate",), max_rounds=1)
    _check_refinement(got, want, str(tmp_path / "rel"), "one.txt")
    # (measured on the CPU before any GPU run: the best relocation gains at most 1.0e-2 absolute on these three
    # arrangements and the inversion at least 9.9e-2, so one relocation stays 8.9e-2 or more short: 5e-2 is asserted)
    assert got[2][chrom]["moves"] == 1 and gold - got[2][chrom]["after"] > 5e-2 and not got[2][chrom]["converged"]
    # the cap: one round on the two-fault start applies the inversion and reports not converged
    got = _refine(paths, groups, str(tmp_path / "two.txt"), str(tmp_path / "cap"), maxRounds=1)
    want = _greedy_all(name, paths, groups, two, chrom, max_rounds=1)
    _check_refinement(got, want, str(tmp_path / "cap"), "two.txt")
    assert got[2][chrom]["moves"] == 1 and not got[2][chrom]["converged"]
    with open(str(tmp_path / "cap" / "refine_summary.tsv")) as fh:
        assert fh.read().splitlines()[chrom + 1].endswith("\tno")


@pytest.mark.parametrize("name", ["n600", "n2000"])
def test_refinement_from_a_golden_order(name, tmp_path):
    paths, groups, orders = _inputs(name, tmp_path)
    golden = read_order_file(orders)
    got = _refine(paths, groups, orders, str(tmp_path / "out"))
    want = _greedy_all(name, paths, groups, golden)
    _check_refinement(got, want, str(tmp_path / "out"), "chromosomeOrders.txt")
    for chrom in [c for n, c in REFINE_CASES if n == name]:
        assert got[2][chrom]["moves"] == 0 and got[2][chrom]["converged"] and got[2][chrom]["rounds"] == 1
    print(name, "moves from the golden order per chromosome:", [s["moves"] for s in got[2]])
    if not got[1]:                                            # zero moves anywhere: the written order file is the input
        with open(str(tmp_path / "out" / "chromosomeOrders.txt")) as fh:
            assert fh.read() == gc.golden_text(name, "chromosomeOrders.txt")
    else:
        kept = read_order_file(str(tmp_path / "out" / "chromosomeOrders.txt"))
        for chrom in [c for n, c in REFINE_CASES if n == name]:
            assert kept[chrom] == golden[chrom]


def _config(tmp_path, paths, groups, n_scaffolds, scan_scaffolds, **extra):
    from hic_genome_assembler_amd import synth
    out = str(tmp_path / "out")
    cfg = synth.write_config(str(tmp_path / "config.txt"), paths, out, str(tmp_path / "plots"), 100000,
                             n_scaffolds=n_scaffolds, scan_scaffolds=scan_scaffolds)
    with open(os.path.join(out, "groups.txt"), "w") as fh, open(groups) as src:
        fh.write(src.read())
    with open(cfg, "a") as fh:                                # a later line replaces an earlier one
        fh.write("".join("%s = %s\n" % kv for kv in dict(extra, chromosomeGroupFile="groups.txt").items()))
    return cfg


def test_part2_with_the_two_config_lines(tmp_path):
    """-part2 with inversionSupportFile and refinedChromosomeOrderFile on n160: the golden outputs as before, and beside
    them the report that supportInversions writes for that order and the order file that refinePart2 writes; without the
    two lines neither file appears."""
    from hic_genome_assembler_amd import refinePart2 as rp, run_hicAssembler as run, supportInversions as si
    name = "n160"
    spec = gc.load_case(name)[0]
    paths, groups, orders = _inputs(name, tmp_path)
    cfg = _config(tmp_path, paths, groups, spec["n_scaffolds"], spec["scan_scaffolds"], inversionSupportFile="inv_part2.txt",
                  refinedChromosomeOrderFile="refined_part2.txt")
    out = str(tmp_path / "out")
    _quiet(run.main, ["-part2", "-config", cfg])
    v = run.readConfigFileToVariables(cfg)
    for key, fn in (("chromosomeOrderFile", "chromosomeOrders.txt"), ("plotOrderFile", "plotOrder.txt")):
        with open(v[key]) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn
    _quiet(si.main, ["-config", cfg, "-chromosomeOrderFile", orders, "-out", os.path.join(out, "inv_cli.txt")])
    _quiet(rp.main, ["-config", cfg, "-chromosomeOrderFile", orders, "-out", os.path.join(out, "refined_cli")])
    for a, b in (("inv_part2.txt", "inv_cli.txt"), ("refined_part2.txt", os.path.join("refined_cli", "chromosomeOrders.txt"))):
        with open(os.path.join(out, a)) as fa, open(os.path.join(out, b)) as fb:
            text = fa.read()
            assert text == fb.read() and text
    # without the two lines: the same golden outputs and nothing else
    plain = tmp_path / "plain"
    plain.mkdir()
    cfg2 = _config(plain, paths, groups, spec["n_scaffolds"], spec["scan_scaffolds"])
    _quiet(run.main, ["-part2", "-config", cfg2])
    v2 = run.readConfigFileToVariables(cfg2)
    for key, fn in (("chromosomeOrderFile", "chromosomeOrders.txt"), ("plotOrderFile", "plotOrder.txt")):
        with open(v2[key]) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn
    assert not [f for f in os.listdir(str(plain / "out")) if "inv" in f or "refined" in f]
