"""Junction support on the GPU (k_junctions.hip through hicmi_junction_sums; orderGenome.junctionSupport,
supportJunctions.py) against the NumPy restatement of tests/junction_reference.py.

Tolerances, fixed before any run: a sum within 1e-10 relative of the reference's (the project's bound for Part 2 scores;
every term is non-negative, so nothing cancels); two default calls compared with ==; the default path against
HICMI_JUNCTIONS_PLAIN=1 within 1e-10.  J and rel are a sum divided by host-side constants, so they carry the same bound;
every other field of the report (picks, verdicts, counts) is compared for equality."""
import contextlib
import io
import os

import numpy as np
import pytest

import golden_cases as gc
import junction_reference as ref
from support_reference import read_group_file, read_order_file, write_order_file

pytestmark = pytest.mark.gpu

REL = 1e-10
GOLDEN = [n for n in gc.case_names() if os.path.exists(os.path.join(gc.GOLDEN_DIR, n, "chromosomeOrders.txt"))]
JOINS = {"n160": 0, "n160_numba": 0, "n500_sparse": 1, "n300_edges": 4, "n600": 4, "n400_default": 6, "n2000": 8}
RESTORED = ("n2000", "n300_edges", "n500_sparse", "n600")     # -joined gives the planted chromosome count
SLAB = 64                                                     # JN_SLAB_ROWS of hicmi_internal.h


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    monkeypatch.delenv("HICMI_JUNCTIONS_PLAIN", raising=False)


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _golden_files(name):
    return [os.path.join(gc.GOLDEN_DIR, name, fn) for fn in ("chromosomeGroups.txt", "chromosomeOrders.txt")]


def _worst(got, exp):
    exp = np.asarray(exp, dtype=np.float64)
    err = np.abs(np.asarray(got) - exp)
    return float(np.max(np.where(exp != 0, err / np.where(exp != 0, np.abs(exp), 1.0), np.where(err == 0, 0.0, np.inf)))) \
        if len(exp) else 0.0


def _golden_records(name, window):
    """bins and records of a golden ordering on the case's whole map (matrix index = bin ID - 1)."""
    from hic_genome_assembler_amd import orderGenome as p2
    lay = gc.load_case(name)[3]
    where = {int(b): i for i, b in enumerate(lay.bin_ids)}
    groups, orders = _golden_files(name)
    chroms = [ref.chromosome_sides(rows, arr, where) for rows, arr in zip(read_group_file(groups), read_order_file(orders))]
    bins, lengths, bounds = [], [], []
    for chrom in chroms:
        sizes = [len(idx) for _n, idx in chrom]
        bins.extend(i for _n, idx in chrom for i in idx)
        lengths.append(sum(sizes))
        bounds.append(list(np.cumsum(sizes)[:-1]))
    return np.array(bins, np.int32), p2.junction_records(lengths, bounds, window)["rec"]


@pytest.mark.parametrize("name", GOLDEN)
def test_every_record_of_the_golden_orderings(name, monkeypatch):
    from hic_genome_assembler_amd import _lib
    c = gc.load_case(name)[4]
    with _lib.Context(0) as ctx:
        ctx.set_contacts(c)
        for window in (16, 0):
            bins, rec = _golden_records(name, window)
            exp = ref.record_sums(c, bins, rec)
            got = ctx.junction_sums(bins, rec)
            again = ctx.junction_sums(bins, rec)
            monkeypatch.setenv("HICMI_JUNCTIONS_PLAIN", "1")
            plain = ctx.junction_sums(bins, rec)
            monkeypatch.delenv("HICMI_JUNCTIONS_PLAIN")
            print("%s window %d: %d records, largest relative error %.3e (bound %.0e), PLAIN %.3e, default vs PLAIN %.3e"
                  % (name, window, len(rec), _worst(got, exp), REL, _worst(plain, exp), _worst(got, plain)))
            assert len(rec) > 0 and np.all(exp > 0)
            assert np.array_equal(got, again)
            assert _worst(got, exp) <= REL and _worst(plain, exp) <= REL and _worst(got, plain) <= REL


# ---- kernel edges: one ~700-bin map, hand-built records in ONE call ------------------------------------
N_EDGE = 701
LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257)     # the lane counts and the slab size, by one either way


def _edge_map(seed=3):
    """Asymmetric on purpose: a kernel that reads M[B][A] for M[A][B] fails."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(rng.random((N_EDGE, N_EDGE)) * np.exp(rng.normal(0.0, 2.0, (N_EDGE, N_EDGE))))


def _edge_records(pool=None, seed=4):
    """(bins, rec): two permutations of ``pool`` (default: every bin) listed one after the other, and records of every
    length pair of LENGTHS x (1, 2, 64, 65, 257), 1 x 600, 600 x 1, a 600 x 650 beside a 1 x 1, both step signs."""
    rng = np.random.default_rng(seed)
    pool = np.arange(N_EDGE) if pool is None else np.asarray(pool)
    bins = np.concatenate([rng.permutation(pool), rng.permutation(pool)]).astype(np.int32)
    n_listed = len(bins)
    shapes = [(la, lb) for la in LENGTHS for lb in (1, 2, 64, 65, 257)]
    shapes += [(1, 600), (600, 1), (600, 650), (1, 1), (SLAB * 3 - 1, 3), (SLAB * 3, 3), (SLAB * 3 + 1, 3)]
    rec = []
    for k, (la, lb) in enumerate(shapes):
        ta, tb = (1, -1)[k % 2], (1, -1)[(k // 2) % 2]
        sa = int(rng.integers(0, n_listed - la + 1)) + (la - 1 if ta < 0 else 0)
        sb = int(rng.integers(0, n_listed - lb + 1)) + (lb - 1 if tb < 0 else 0)
        rec.append((sa, ta, la, sb, tb, lb))
    assert len(pool) >= 650
    return bins, np.array(rec, np.int64)


def _check_edges(ctx, M, bins, rec, label, monkeypatch):
    exp = ref.record_sums(M, bins, rec)
    got = ctx.junction_sums(bins, rec)
    again = ctx.junction_sums(bins, rec)
    monkeypatch.setenv("HICMI_JUNCTIONS_PLAIN", "1")
    plain = ctx.junction_sums(bins, rec)
    monkeypatch.delenv("HICMI_JUNCTIONS_PLAIN")
    print("%s: %d records, largest relative error %.3e (bound %.0e), PLAIN %.3e, default vs PLAIN %.3e"
          % (label, len(rec), _worst(got, exp), REL, _worst(plain, exp), _worst(got, plain)))
    assert np.array_equal(got, again)
    assert _worst(got, exp) <= REL and _worst(plain, exp) <= REL and _worst(got, plain) <= REL
    return got


def test_kernel_edges_in_one_call(monkeypatch):
    from hic_genome_assembler_amd import _lib
    M = _edge_map()
    bins, rec = _edge_records()
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M)
        whole = _check_edges(ctx, M, bins, rec, "fp64 upload", monkeypatch)
        # n_rec = 1, and the order of a sum depends on its record alone: every record on its own gives the call's bits
        for r in (0, len(rec) - 5, len(rec) - 4):               # 1 x 1 sides, the 600 x 650, the 1 x 1
            alone = ctx.junction_sums(bins, rec[r:r + 1])
            assert alone.shape == (1,) and alone[0] == whole[r]
        assert ctx.junction_sums(bins, rec[:0]).shape == (0,)


@pytest.mark.parametrize("ld", [720, 733])
def test_adopted_matrix_with_a_leading_dimension(ld, monkeypatch):
    import torch
    from hic_genome_assembler_amd import _lib
    M = _edge_map(5)
    bins, rec = _edge_records(seed=6)
    t = torch.full((N_EDGE, ld), float("nan"), dtype=torch.float64, device="cuda:0")
    t[:, :N_EDGE] = torch.as_tensor(M, device="cuda:0")
    torch.cuda.synchronize()
    with _lib.Context(0) as ctx:
        ctx.set_contacts_device(t.data_ptr(), N_EDGE, ld, keepalive=t)
        _check_edges(ctx, M, bins, rec, "adopted, ld %d" % ld, monkeypatch)


def test_fp32_upload(monkeypatch):
    from hic_genome_assembler_amd import _lib
    M32 = _edge_map(7).astype(np.float32)
    bins, rec = _edge_records(seed=8)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M32)
        _check_edges(ctx, M32.astype(np.float64), bins, rec, "fp32 upload", monkeypatch)


def test_zero_rows_before_and_after_compact(monkeypatch):
    from hic_genome_assembler_amd import _lib
    M = _edge_map(9)
    dead = np.random.default_rng(10).choice(N_EDGE, 40, replace=False)
    M[dead, :] = 0.0
    M[:, dead] = 0.0
    keep = np.setdiff1d(np.arange(N_EDGE), dead).astype(np.int32)
    bins, rec = _edge_records(seed=11)                        # sides run over the zero rows too: their terms are 0.0
    bins_k, rec_k = _edge_records(pool=np.arange(len(keep)), seed=12)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M)
        _check_edges(ctx, M, bins, rec, "zero rows, before compact", monkeypatch)
        ctx.compact(keep)
        _check_edges(ctx, M[np.ix_(keep, keep)], bins_k, rec_k, "zero rows, after compact", monkeypatch)
        with pytest.raises(_lib.HicmiError):                   # a bin of the old numbering is outside the compacted map
            ctx.junction_sums(np.array([len(keep)], np.int32), np.array([[0, 1, 1, 0, 1, 1]], np.int64))


def test_a_map_of_ones_by_values_only(monkeypatch):
    """Every J of a map of ones is 1 up to rounding, so no pick is asserted there: the sums are the norms."""
    from hic_genome_assembler_amd import _lib, orderGenome as p2
    M = np.ones((N_EDGE, N_EDGE))
    bins, rec = _edge_records(seed=13)
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M)
        got = _check_edges(ctx, M, bins, rec, "map of ones", monkeypatch)
    J = np.array([s / p2.junction_norm(r[2], r[5]) for s, r in zip(got, rec)])
    print("map of ones: largest |J - 1| %.3e" % float(np.max(np.abs(J - 1.0))))
    assert np.max(np.abs(J - 1.0)) <= REL


def test_refusals_leave_the_context_as_it_was():
    from hic_genome_assembler_amd import _lib
    M = _edge_map(14)
    bins, rec = _edge_records(seed=15)
    n_listed = len(bins)
    ok = np.array([[0, 1, 5, n_listed - 1, -1, 7]], np.int64)

    def bad_record(**kw):
        r = dict(sa=0, ta=1, la=5, sb=n_listed - 1, tb=-1, lb=7)
        r.update(kw)
        return np.array([[r["sa"], r["ta"], r["la"], r["sb"], r["tb"], r["lb"]]], np.int64)
    cases = [("a length of 0", bins, bad_record(la=0)), ("a negative length", bins, bad_record(lb=-3)),
             ("a step of 2", bins, bad_record(ta=2)), ("a step of 0", bins, bad_record(tb=0)),
             ("a start below 0", bins, bad_record(sa=-1)), ("a start past the end", bins, bad_record(sb=n_listed)),
             ("a side running past the end", bins, bad_record(sa=n_listed - 3)),
             ("a side running below 0", bins, bad_record(sb=5)),
             ("a side longer than bins", bins, bad_record(la=n_listed + 1)),
             ("a bin equal to n", np.where(np.arange(n_listed) == 17, N_EDGE, bins).astype(np.int32), ok),
             ("a negative bin", np.where(np.arange(n_listed) == n_listed - 1, -1, bins).astype(np.int32), ok),
             ("a bad record behind good ones", bins, np.concatenate([rec, bad_record(ta=-2)]))]
    with _lib.Context(0) as empty:
        with pytest.raises(_lib.HicmiError) as err:
            empty.junction_sums(bins, ok)
        assert "error -1" in str(err.value)                    # HICMI_EINVAL: no matrix set
    with _lib.Context(0) as ctx:
        ctx.set_contacts(M)
        first = ctx.junction_sums(bins, rec)
        for label, b, r in cases:
            with pytest.raises(_lib.HicmiError) as err:
                ctx.junction_sums(b, r)
            assert "error -1" in str(err.value), label          # HICMI_EINVAL
            assert np.array_equal(ctx.junction_sums(bins, rec), first), label
        assert _worst(first, ref.record_sums(M, bins, rec)) <= REL


# ---- the report, the picks and the files on the golden orderings ---------------------------------------
def _inputs(name, tmp_path):
    paths = _quiet(gc.write_case_files, name, str(tmp_path))
    groups, orders = _golden_files(name)
    return paths, groups, orders


def _junctions(paths, groups, orders, out, **kw):
    from hic_genome_assembler_amd import supportJunctions as sj
    return _quiet(sj.runJunctions, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], groups, orders,
                  out, **kw)


def _reference(paths, groups, orders, window=16, min_rel=0.25):
    """ref.analyse on the matrix the product reads from the HiC-Pro files (the grouped bins only)."""
    from hic_genome_assembler_amd import orderGenome as p2
    from hic_genome_assembler_amd.hostio import initiateLoci, read_contact_matrix
    binList = _quiet(initiateLoci, paths["hicProBedFile"], paths["hicProBiasFile"],
                     binID_dict=p2.readGroupingsToValidBins(groups))
    host = np.ascontiguousarray(_quiet(read_contact_matrix, paths["hicProMatrixFile"], binList), dtype=np.float64)
    where = {b.ID: i for i, b in enumerate(binList)}
    chroms = [ref.chromosome_sides(rows, arr, where) for rows, arr in zip(read_group_file(groups), read_order_file(orders))]
    exp = ref.analyse(host, chroms, window, min_rel)
    exp["end_bin"] = [binList[chroms[e // 2][-1 if e % 2 else 0][1][-1 if e % 2 else 0]].ID for e in range(2 * len(chroms))]
    return exp


def _is_float(tok):
    """repr of a float: it holds a '.', an exponent or inf / nan, which no count and no scaffold name that parses does."""
    try:
        float(tok)
    except ValueError:
        return False
    return not tok.lstrip("-").isdigit()


def _same_report(text, expected):
    """Every token that is not a float equal; every float within REL.  Returns the largest relative difference."""
    worst = 0.0
    got_lines, exp_lines = text.splitlines(), expected.splitlines()
    assert len(got_lines) == len(exp_lines)
    for g, e in zip(got_lines, exp_lines):
        gt, et = g.replace("\t", " ").split(" "), e.replace("\t", " ").split(" ")
        assert len(gt) == len(et), (g, e)
        for a, b in zip(gt, et):
            if _is_float(b) and _is_float(a):
                worst = max(worst, abs(float(a) - float(b)) / abs(float(b)) if float(b) else abs(float(a)))
            else:
                assert a == b, (g, e)
    assert worst <= REL
    return worst


@pytest.mark.parametrize("name", GOLDEN)
def test_report_picks_and_joins_on_the_golden_orderings(name, tmp_path):
    lay = gc.load_case(name)[3]
    paths, groups, orders = _inputs(name, tmp_path)
    joined = str(tmp_path / "joined")
    res = _junctions(paths, groups, orders, str(tmp_path / "junctions.txt"), joinedDir=joined, fullDir=str(tmp_path / "full"))
    exp = _reference(paths, groups, orders)
    with open(str(tmp_path / "junctions.txt")) as fh:
        report = fh.read()
    worst = _same_report(report, ref.report_text(exp))
    print("%s: %d internal junctions, %d ends, largest relative difference of a float in the report %.3e (bound %.0e)"
          % (name, len(res["internal"]), len(res["ends"]), worst, REL))
    assert _worst(res["sums"], exp["sums"]) <= REL
    # picks and verdicts, as data
    assert [r["best"] for r in res["ends"]] == [r["best"] for r in exp["ends"]]
    assert [r["second"] for r in res["ends"]] == [r["second"] for r in exp["ends"]]
    assert [r["verdict"] or "NA" for r in res["ends"]] == [r["verdict"] for r in exp["ends"]]
    assert [(e, f) for e, f, _J in res["joinable"]] == [(2 * a[0] + a[1], 2 * b[0] + b[1]) for a, b, _J in exp["joins"]]
    assert np.array_equal(np.isnan(res["table"]), np.isnan(exp["table"])) and np.array_equal(res["table"], res["table"].T,
                                                                                             equal_nan=True)
    # the counts found with the NumPy restatement when the statistic was proposed; the reference must reproduce them
    assert len(exp["joins"]) == JOINS[name] and len(res["joinable"]) == JOINS[name]
    assert not exp["weak"] and not res["weak"]
    pos = {int(b): (int(lay.chrom_of_bin[i]), int(lay.pos_of_bin[i])) for i, b in enumerate(lay.bin_ids)}
    for e, f, _J in res["joinable"]:
        (ce, pe), (cf, pf) = pos[exp["end_bin"][e]], pos[exp["end_bin"][f]]
        assert ce == cf and abs(pe - pf) <= 2, (e, f, pe, pf)
    # -joined: the reference's joins applied to plain lists, and a valid pair of files
    arr = read_order_file(orders)
    want, members, dropped = ref.join_plain(arr, exp["joins"])
    assert not dropped
    got = read_order_file(os.path.join(joined, "chromosomeOrders.txt"))
    assert got == want
    if name in RESTORED:
        assert len(got) == len(set(lay.chrom_of_bin.tolist()))
    new_groups = read_group_file(os.path.join(joined, "chromosomeGroups.txt"))
    old_groups = read_group_file(groups)
    assert [sorted(map(tuple, g)) for g in new_groups] == [sorted(tuple(r) for c, _rev in mem for r in old_groups[c])
                                                           for mem in members]
    with open(os.path.join(joined, "joins.log")) as fh:
        assert len(fh.read().splitlines()) == JOINS[name]
    with open(str(tmp_path / "full" / "junctions.ends.tsv")) as fh:
        assert len(fh.read().splitlines()) == 2 * len(arr) + 1
    with open(groups) as fa, open(os.path.join(gc.GOLDEN_DIR, name, "chromosomeGroups.txt")) as fb:
        assert fa.read() == fb.read()                          # the inputs are only read


def _lines_of(group_file):
    """Per group its lines verbatim."""
    with open(group_file) as fh:
        lines = fh.read().splitlines(keepends=True)
    out = []
    for k, line in enumerate(lines):
        if k == 0 or line.startswith("#"):
            out.append([])
        else:
            out[-1].append(line)
    return out


def _write_groups(path, groups):
    with open(path, "w") as fh:
        for k, lines in enumerate(groups):
            fh.write("### Chromosome group %d ###\n" % (k + 1) + "".join(lines))


def split_inputs(tmp, groups, orders, chrom, swap=False):
    """The golden files with chromosome ``chrom`` split at its middle scaffold boundary into two chromosomes that stand
    where it stood, the first piece first (``swap``: the second piece first).  A group holds whole lines of the group
    file in the file's order."""
    arr, lines = read_order_file(orders), _lines_of(groups)
    mid = len(arr[chrom]) // 2
    first = {n for n, _o in arr[chrom][:mid]}
    pieces = [(arr[chrom][:mid], [ln for ln in lines[chrom] if ln.split("\t")[1].strip() in first]),
              (arr[chrom][mid:], [ln for ln in lines[chrom] if ln.split("\t")[1].strip() not in first])]
    if swap:
        pieces.reverse()
    os.makedirs(tmp, exist_ok=True)
    g2, o2 = os.path.join(tmp, "chromosomeGroups.txt"), os.path.join(tmp, "chromosomeOrders.txt")
    write_order_file(o2, arr[:chrom] + [p[0] for p in pieces] + arr[chrom + 1:])
    _write_groups(g2, lines[:chrom] + [p[1] for p in pieces] + lines[chrom + 1:])
    return g2, o2


def concatenated_inputs(tmp, groups, orders):
    """The golden files with chromosomes 1 and 2 concatenated."""
    arr, lines = read_order_file(orders), _lines_of(groups)
    os.makedirs(tmp, exist_ok=True)
    g2, o2 = os.path.join(tmp, "chromosomeGroups.txt"), os.path.join(tmp, "chromosomeOrders.txt")
    write_order_file(o2, [arr[0] + arr[1]] + arr[2:])
    _write_groups(g2, [lines[0] + lines[1]] + lines[2:])
    return g2, o2, len(arr[0]) - 1


def _same_files(directory, name, files):
    for fn in files:
        with open(os.path.join(directory, fn)) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn


@pytest.mark.parametrize("chrom,swap", [(0, False), (1, False), (2, False), (3, False), (3, True)])
def test_a_split_chromosome_is_joined_again(chrom, swap, tmp_path):
    """n160's golden files with one chromosome split at its middle scaffold boundary: exactly that pair is joinable, and
    -joined gives the golden order and plot-order files back byte for byte.  A group of the group file holds whole
    scaffold blocks in an order of Part 1's, which the two pieces interleave; a joined group is its members' lines,
    lowest-numbered member first, so the group file comes back as the same groups of the same lines for every split, and
    byte for byte where the pieces are numbered in the order their lines stand in the file: chromosome 4, whose second
    piece stands first there (``swap``: also a join whose reading direction starts at the higher-numbered member)."""
    name = "n160"
    paths, groups, orders = _inputs(name, tmp_path)
    g2, o2 = split_inputs(str(tmp_path / "split"), groups, orders, chrom, swap)
    joined = str(tmp_path / "joined")
    res = _junctions(paths, g2, o2, str(tmp_path / "junctions.txt"), joinedDir=joined)
    pair = (2 * chrom, 2 * chrom + 3) if swap else (2 * chrom + 1, 2 * chrom + 2)
    print("split of chromosome %d: joinable %s, rel %s" % (chrom + 1, res["joinable"],
                                                             [r["rel"] for r in res["ends"] if r["verdict"] == "joinable"]))
    assert [(e, f) for e, f, _J in res["joinable"]] == [pair]
    assert [e for e, r in enumerate(res["ends"]) if r["verdict"] == "joinable"] == list(pair)
    assert not res["weak"]
    _same_files(joined, name, ("chromosomeOrders.txt", "plotOrder.txt"))
    got, want = _lines_of(os.path.join(joined, "chromosomeGroups.txt")), _lines_of(groups)
    assert [sorted(g) for g in got] == [sorted(g) for g in want]
    if swap:
        _same_files(joined, name, ("chromosomeGroups.txt",))
    assert len(_lines_of(g2)) == len(want) + 1                # the input is only read


def test_two_concatenated_chromosomes_are_cut_again(tmp_path):
    """n160's golden files with chromosomes 1 and 2 concatenated: exactly that junction is weak (0.004 times the median
    when the statistic was proposed), and -cut gives the golden files back byte for byte."""
    name = "n160"
    paths, groups, orders = _inputs(name, tmp_path)
    g2, o2, at = concatenated_inputs(str(tmp_path / "cat"), groups, orders)
    cut = str(tmp_path / "cut")
    res = _junctions(paths, g2, o2, str(tmp_path / "junctions.txt"), cutDir=cut)
    rels = [r["rel"] for r in res["internal"] if r["verdict"] == "weak"]
    print("concatenation of chromosomes 1 and 2: weak %s, rel %s" % (res["weak"], rels))
    assert res["weak"] == [(0, at)] and rels[0] < 0.01
    assert not res["joinable"]
    _same_files(cut, name, ("chromosomeOrders.txt", "plotOrder.txt", "chromosomeGroups.txt"))
    with open(os.path.join(cut, "cuts.log")) as fh:
        assert len(fh.read().splitlines()) == 1


def test_support_and_refinement_accept_the_joined_files(tmp_path):
    from hic_genome_assembler_amd import refinePart2 as rp, supportPart2 as sp
    name = "n600"
    lay = gc.load_case(name)[3]
    paths, groups, orders = _inputs(name, tmp_path)
    joined = str(tmp_path / "joined")
    _junctions(paths, groups, orders, str(tmp_path / "junctions.txt"), joinedDir=joined)
    g2, o2, p2_ = [os.path.join(joined, fn) for fn in ("chromosomeGroups.txt", "chromosomeOrders.txt", "plotOrder.txt")]
    planted = len(set(lay.chrom_of_bin.tolist()))
    support = _quiet(sp.runSupport, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"], g2, o2,
                     str(tmp_path / "support.txt"))
    assert len(support) == planted and [r["names"] for r in support] == [[n for n, _o in a] for a in read_order_file(o2)]
    refined, _log, summary = _quiet(rp.runRefine, paths["hicProBedFile"], paths["hicProBiasFile"], paths["hicProMatrixFile"],
                                    g2, o2, p2_, str(tmp_path / "refined"))
    assert len(refined) == planted == len(summary)
    assert sorted(s.name for g in refined for s in g) == sorted(n for a in read_order_file(orders) for n, _o in a)


def _config(tmp_path, paths, spec, **extra):
    from hic_genome_assembler_amd import synth
    cfg = synth.write_config(str(tmp_path / "config.txt"), paths, str(tmp_path / "out"), str(tmp_path / "plots"), 100000,
                             min_size=spec["min_size"], psig=spec["psig"], n_scaffolds=spec["n_scaffolds"],
                             scan_scaffolds=spec["scan_scaffolds"])
    with open(cfg, "a") as fh:
        fh.write("".join("%s = %s\n" % kv for kv in extra.items()))
    return cfg


def test_part2_with_the_two_config_lines(tmp_path):
    """-part1 -part2 on n160 with junctionSupportFile and joinedFilesDirectory: the six golden outputs as before, the
    report that supportJunctions writes for that order, and the joined files; without the two lines the same outputs,
    nothing else written and nothing else printed."""
    from hic_genome_assembler_amd import run_hicAssembler as run, supportJunctions as sj
    name = "n160"
    spec = gc.load_case(name)[0]
    paths = _quiet(gc.write_case_files, name, str(tmp_path))
    with_lines = tmp_path / "with"
    with_lines.mkdir()
    cfg = _config(with_lines, paths, spec, junctionSupportFile="junctions_part2.txt", joinedFilesDirectory="joined_part2")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        run.main(["-part1", "-part2", "-config", cfg])
    v = run.readConfigFileToVariables(cfg)
    keys = ("dendrogramOrderFile", "binGroupFile", "assessmentFile", "chromosomeGroupFile", "chromosomeOrderFile", "plotOrderFile")
    for key, fn in zip(keys, gc.OUTPUT_FILES):
        with open(v[key]) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn
    out = str(with_lines / "out")
    _quiet(sj.main, ["-config", cfg, "-out", os.path.join(out, "junctions_cli.txt"), "-joined", os.path.join(out, "joined_cli")])
    with open(os.path.join(out, "junctions_part2.txt")) as fa, open(os.path.join(out, "junctions_cli.txt")) as fb:
        text = fa.read()
        assert text == fb.read() and text.startswith("### reference ")
    for fn in sorted(os.listdir(os.path.join(out, "joined_cli"))):
        with open(os.path.join(out, "joined_part2", fn)) as fa, open(os.path.join(out, "joined_cli", fn)) as fb:
            assert fa.read() == fb.read(), fn
    assert sorted(os.listdir(os.path.join(out, "joined_part2"))) == sorted(
        [os.path.basename(v[k]) for k in keys[3:]] + ["joins.log"])
    # without the two lines
    plain = tmp_path / "plain"
    plain.mkdir()
    cfg2 = _config(plain, paths, spec)
    buf2 = io.StringIO()
    with contextlib.redirect_stdout(buf2):
        run.main(["-part1", "-part2", "-config", cfg2])
    v2 = run.readConfigFileToVariables(cfg2)
    for key, fn in zip(keys, gc.OUTPUT_FILES):
        with open(v2[key]) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn
    extra = set(os.listdir(out)) - set(os.listdir(str(plain / "out")))
    assert extra == {"junctions_part2.txt", "junctions_cli.txt", "joined_part2", "joined_cli"}

    assert "Junction support written" in buf.getvalue() and "Chromosome ends joined" in buf.getvalue()
    assert "Junction" not in buf2.getvalue() and "joined" not in buf2.getvalue()
