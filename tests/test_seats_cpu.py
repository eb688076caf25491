"""supportSeats and polishOrder's relocate rounds without a GPU: tests/seats_reference.py against its own
brute-force table, csrc/seats.h built as host code with the sanitizers and compared line by line with the reference, the
defining equivalence with anchoring on the layout without one scaffold, the invariants of the table, the planted displaced
case, and the command lines - the nine verdicts, the ``-moved`` file, the relocate rounds and the refusals - on a NumPy
stand-in context.  Every comparison is of integers, bit for bit."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import anchor_reference as aref
import ends_reference as eref
import liftmap_reference as lref
import pairs_reference as pref
import seats_reference as ref
import test_anchor_cpu as anchor_cases
import test_ends_cpu as ends_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")
SEEDS = range(12)


def _pairs(rows):
    sa, pa, sb, pb = zip(*rows)
    return (np.array(sa, np.int32), np.array(pa, np.int64), np.array(sb, np.int32), np.array(pb, np.int64))


def _read(path):
    with open(path, newline="") as fh:
        return fh.read()


def _random_case(seed):
    sizes, tables, pairs, window, _reach = ends_cases._random_case(seed)
    return sizes, tables, pairs, window


# ---- the reference against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_reference_table_equals_the_brute_force_table(seed):
    sizes, tables, pairs, window = _random_case(seed)
    T, counters = ref.table(pairs, sizes, tables, window)
    bT, bc = ref.brute_table(pairs, sizes, tables, window)
    assert T.dtype == np.uint64 and T.shape == bT.shape and T.tobytes() == bT.tobytes() and counters.tolist() == bc.tolist()
    assert len(T) == ref.number_blocks(sizes, tables)[1]


def test_the_random_cases_hold_every_kind_of_pair():
    total = np.zeros(5, np.uint64)
    for seed in SEEDS:
        sizes, tables, pairs, window = _random_case(seed)
        total += ref.table(pairs, sizes, tables, window)[1]
    assert (total > 20).all(), total


def test_blocks_and_a_pair_against_a_hand_worked_case():
    # Chr_1 = c- (7 bases), b- (1), a+ (5); Chr_2 = d+ (3), f (no base); e is dropped
    tables = lref.layout(ends_cases.CHROMS, ends_cases.SIZES, 100, drop_unplaced=True)
    first, n = ref.number_blocks(ends_cases.SIZES, tables)
    assert first.tolist() == [0, 14, 28, 42, -1, -1] and n == 3 * (2 + 12) + (2 + 4)
    # window 2; a pair of base 5 of a (its second half, its RIGHT zone) with base 7 of c (reversed: its first base as it
    # lies, LEFT; in c's own + coordinates its second half)
    T, counters = ref.table(_pairs([(0, 5, 2, 7)]), ends_cases.SIZES, tables, 2)
    want = np.zeros(n, np.uint64)
    want[0 + 0] = want[28 + 0] = 1                                         # both lie in Chr_1
    want[0 + 2 + 0 * 4 + 1 * 2 + ref.LEFT] = 1                             # a's block: row of c (local rank 0), a's half 1, c's zone
    want[28 + 2 + 2 * 4 + 1 * 2 + ref.RIGHT] = 1                           # c's block: row of a (local rank 2), c's half 1, a's zone
    assert T.tobytes() == want.tobytes() and counters.tolist() == [1, 0, 0, 0, 0]
    # the middle base of a is in no zone at window 2: only c's block gets no gap counter
    T, counters = ref.table(_pairs([(2, 7, 0, 3)]), ends_cases.SIZES, tables, 2)
    assert int(T.sum()) == 3 and T[0 + 2 + 0 * 4 + 0 * 2 + ref.LEFT] == 1 and counters.tolist() == [1, 0, 0, 0, 0]
    T, counters = ref.table(_pairs([(2, 4, 0, 3), (0, 1, 3, 1), (3, 1, 3, 2), (4, 1, 0, 1)]), ends_cases.SIZES, tables, 2)
    assert counters.tolist() == [0, 1, 1, 1, 1] and int(T.sum()) == 4 and T[0 + 1] == 1 and T[42 + 0] == 1


# ---- seats.h as host code under the sanitizers ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("seats") / "seats_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "seats_host_check.cpp"), "-o", exe])

    def run(path, sizes, tables, window, pairs, print_table=True):
        seq, off, rev, seq_sizes = tables
        lines = ["T %d %d %d %d" % (len(sizes), len(seq_sizes), window, print_table)]
        lines += ["%d %d %d %d" % row for row in zip(np.asarray(sizes).tolist(), seq.tolist(), off.tolist(), rev.tolist())]
        lines += [" ".join(str(int(x)) for x in seq_sizes), "P %d" % len(pairs[0])]
        lines += ["%d %d %d %d" % row for row in zip(*(np.asarray(x).tolist() for x in pairs))]
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        # an ordinary child process, nothing preloaded
        done = subprocess.run([exe, path], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        return done.stdout.splitlines()
    return run


def _expected_lines(sizes, tables, window, pairs):
    first, n = ref.number_blocks(sizes, tables)
    kind, index = ref.classify(pairs, sizes, tables, window)
    T, counters = ref.table(pairs, sizes, tables, window)
    out = ["check 0 ", "table %d" % n] + ["first %d" % r for r in first]
    out += ["pair %d %d %d %d %d" % ((k,) + tuple(i)) for k, i in zip(kind.tolist(), index.tolist())]
    return out + ["counters " + " ".join(str(c) for c in counters.tolist())] + ["t %d" % c for c in T.tolist()]


@pytest.mark.parametrize("seed", SEEDS)
def test_native_blocks_kinds_and_table_under_the_sanitizers(seed, host_check, tmp_path):
    sizes, tables, pairs, window = _random_case(seed)
    assert host_check(str(tmp_path / "case.txt"), sizes, tables, window, pairs) == _expected_lines(sizes, tables, window, pairs)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", [0, 100])
def test_native_hand_worked_assembly_every_base_with_every_base(gap, drop, host_check, tmp_path):
    sizes = ends_cases.SIZES
    tables = lref.layout(ends_cases.CHROMS, sizes, gap, drop_unplaced=drop)
    ends = [(s, p) for s in range(5) for p in range(1, int(sizes[s]) + 1)]
    pairs = _pairs([a + b for a in ends for b in ends])
    for window in (1, 2, 3, 100):
        got = host_check(str(tmp_path / "case.txt"), sizes, tables, window, pairs)
        assert got == _expected_lines(sizes, tables, window, pairs)
        T, counters = ref.table(pairs, sizes, tables, window)
        bT, bc = ref.brute_table(pairs, sizes, tables, window)
        assert T.tobytes() == bT.tobytes() and counters.tolist() == bc.tolist()
    # e (4 bases) is a sequence of its own unless it is dropped: a chromosome of one scaffold
    assert got[1] == "table %d" % (3 * (2 + 12) + (2 + 4) if drop else 3 * (3 + 12) + (3 + 4) + (3 + 4))


def test_native_positions_above_2_to_the_32_under_the_sanitizers(host_check, tmp_path):
    L = 2 ** 33
    big = 2 ** 62 - 5
    sizes = np.array([L, L + 1, L, 5, big], dtype=np.int64)
    tables = lref.layout([[(0, "+"), (1, "-"), (2, "+")], [(4, "-")]], sizes, 100)
    for window in (1, 2 ** 20, 2 ** 32, 2 ** 32 + 1, 2 ** 62):
        mid = L // 2
        edge = [1, 2, window, window + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, mid, mid + 1, mid + 2, L - window, L - window + 1, L - 1, L]
        ends = [(s, p) for s in range(3) for p in edge if 1 <= p <= sizes[s]] + [(1, L + 1), (3, 1), (3, 5), (4, 1), (4, big), (4, big // 2), (4, big - big // 2)]
        pairs = _pairs([a + b for a in ends for b in ends])
        assert host_check(str(tmp_path / "case.txt"), sizes, tables, window, pairs) == _expected_lines(sizes, tables, window, pairs)


def test_native_no_pair_and_a_chromosome_of_one_scaffold(host_check, tmp_path):
    sizes = np.array([9, 4, 6], dtype=np.int64)
    tables = lref.layout([[(1, "-")], [(2, "+"), (0, "+")]], sizes, 100)
    none = tuple(np.zeros(0, t) for t in (np.int32, np.int64, np.int32, np.int64))
    got = host_check(str(tmp_path / "case.txt"), sizes, tables, 3, none)
    assert got == ["check 0 ", "table 26", "first 0", "first 10", "first 16", "counters 0 0 0 0 0"] + ["t 0"] * 26
    # the one scaffold of Chr_1 has a row of its own and nothing else: a pair with it is trans
    pairs = _pairs([(1, 1, 0, 9), (2, 1, 1, 4)])
    got = host_check(str(tmp_path / "case.txt"), sizes, tables, 3, pairs)
    assert got == _expected_lines(sizes, tables, 3, pairs)
    assert got[5:7] == ["pair %d 11 0 -1 -1" % ref.TRANS, "pair %d 16 11 -1 -1" % ref.TRANS]


def test_native_table_limit_from_both_sides_under_the_sanitizers(host_check, tmp_path):
    none = _pairs([(0, 1, 0, 1)])
    # S scaffolds in the first of n_seq sequences: S (n_seq + 4 S) counters; 2^10 (2^17 - 2^12 + 2^12) = 2^27
    S, n_seq = 2 ** 10, 2 ** 17 - 2 ** 12
    for extra, fit in ((0, True), (1, False)):
        n = S + extra
        assert (n * (n_seq + 4 * n) <= ref.MAX_TABLE) == fit
        sizes = np.ones(n, np.int64)
        tables = lref.layout([[(s, "+") for s in range(n)]] + [[]] * (n_seq - 1), sizes, 0, drop_unplaced=True)
        got = host_check(str(tmp_path / "case.txt"), sizes, tables, 1, none, print_table=False)
        if fit:
            assert ref.number_blocks(sizes, tables)[1] == 2 ** 27
            assert got[:2] == ["check 0 ", "table %d" % 2 ** 27] and got[2:4] == ["first 0", "first %d" % (n_seq + 4 * S)]
            assert got[1 + n:] == ["first %d" % (2 ** 27 - n_seq - 4 * S), "pair %d -1 -1 -1 -1" % ref.SAME, "counters 0 0 0 1 0"]
        else:
            assert ref.number_blocks(sizes, tables)[1] == -1 and got == ["check 0 ", "table -1"]


# ---- the defining equivalence: anchoring on the layout without one scaffold --------------------------------------------------------
def _chromosomes(sizes, tables):
    """The sequences of ``tables`` as lists of (scaffold, orientation) in the order they lie."""
    seq, off, rev, seq_sizes = tables
    return [[(s, "+-"[int(rev[s])]) for s in sorted((s for s in range(len(sizes)) if seq[s] == q), key=lambda s: (int(off[s]), sizes[s] > 0, s))]
            for q in range(len(seq_sizes))]


@pytest.mark.parametrize("seed", SEEDS)
def test_a_block_is_what_anchoring_counts_on_the_layout_without_its_scaffold(seed):
    sizes, tables, pairs, window = _random_case(seed)
    n_seq = len(tables[3])
    chroms = _chromosomes(sizes, tables)
    first, _n = ref.number_blocks(sizes, tables)
    T, _counters = ref.table(pairs, sizes, tables, window)
    seen = 0
    for c in np.flatnonzero(first >= 0).tolist():
        q = int(tables[0][c])
        a, gaps, k_c = ref.own_block(T, first, sizes, tables, c)
        assert not gaps[k_c].any()                                            # the row of c itself stays zero
        for out in (lref.layout([[(s, o) for s, o in chrom if s != c] for chrom in chroms], sizes, 100, drop_unplaced=True),
                    ref.without(tables, c)):
            # the scaffolds the case drops stay dropped: they are candidates of the sequence mode too, c is one among them
            out[0][np.asarray(tables[0]) < 0] = -1
            first1, _n1 = aref.number_blocks(sizes, out)
            T1, _c1 = aref.table(pairs, sizes, out, None, window)
            assert T1[first1[c]:first1[c] + n_seq].tobytes() == a.tobytes()
            if len(gaps) > 1:
                target = np.full(len(sizes), -1, np.int32)
                target[c] = q
                T2, _c2 = aref.table(pairs, sizes, out, target, window)
                assert T2.tobytes() == np.delete(gaps, k_c, axis=0).reshape(-1).tobytes()
                seen += 1
    assert seen >= 2


# ---- invariants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_invariants_of_the_table(seed):
    sizes, tables, pairs, window = _random_case(seed)
    n_seq = len(tables[3])
    first, n = ref.number_blocks(sizes, tables)
    T, counters = ref.table(pairs, sizes, tables, window)
    placed = np.flatnonzero(first >= 0).tolist()
    a = {c: ref.own_block(T, first, sizes, tables, c)[0].astype(np.int64) for c in placed}
    assert int(counters.sum()) == len(pairs[0])
    assert sum(int(x.sum()) for x in a.values()) == 2 * int(counters[ref.SEATED] + counters[ref.MIDDLE] + counters[ref.TRANS])
    by_seq = np.zeros((n_seq, n_seq), np.int64)
    for c in placed:
        by_seq[int(tables[0][c])] += a[c]
    assert np.array_equal(by_seq, by_seq.T)                                   # links of q with q' seen from either side
    sa, pa, sb, pb = pairs
    swapped, swapped_counters = ref.table((sb, pb, sa, pa), sizes, tables, window)
    assert swapped.tobytes() == T.tobytes() and swapped_counters.tolist() == counters.tolist()
    # from a store: the intra pairs come back as same and unlifted
    sT, sc = ref.store_table(pref.keep(pairs), pref.intra(pairs, len(sizes)), sizes, tables, window)
    assert sT.tobytes() == T.tobytes() and sc.tolist() == counters.tolist()


# ---- a stand-in context ------------------------------------------------------------------------------------------------------------
class StandInContext(pref.StandInContext):
    """pairs_reference.StandInContext with the seat-support call answered by the reference."""

    def seats_resident(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window):
        kept, counts, store_sizes = self.store
        assert np.array_equal(store_sizes, np.asarray(sizes, np.int64))
        tables = self._tables(lift_seq, lift_off, lift_rev, seq_sizes)
        T, counters = ref.store_table(kept, counts, store_sizes, tables, window)
        self.calls.append("seats_resident")
        return ref.number_blocks(store_sizes, tables)[0], T, counters


# ---- the planted case ----------------------------------------------------------------------------------------------------------------
DISPLACED = ((0, 2, 9, False), (1, 10, 3, True), (2, 5, 6, False))          # chromosome, place it is taken from, place it lies at, sign changed
W, R, MP, MR = 5000, 2, 4, 2.0


def displaced_chroms(true_chroms):
    chroms = [list(chrom) for chrom in true_chroms]
    for q, i, j, turn in DISPLACED:
        s, o = chroms[q].pop(i)
        chroms[q].insert(j, (s, ("+" if o == "-" else "-") if turn else o))
    return chroms


def _leave_one_out(P, chroms):
    """{scaffold: (verdict, gap, orientation, score, home_score)} and F through anchor_reference alone: every scaffold in
    turn is dropped from the layout and placed again by the rules of placeUnplaced."""
    sizes = P["sizes"]
    tables = lref.layout(chroms, sizes, 100, drop_unplaced=True)
    F = int(eref.table(P["pairs"], sizes, tables, W, R)[0][:, :, eref.RL].sum())
    out = {}
    for q, chrom in enumerate(chroms):
        for k, (c, o_c) in enumerate(chrom):
            less = lref.layout([[(s, o) for s, o in ch if s != c] for ch in chroms], sizes, 100, drop_unplaced=True)
            first1, _n = aref.number_blocks(sizes, less)
            a = [int(x) for x in aref.table(P["pairs"], sizes, less, None, W)[0][first1[c]:first1[c] + len(chroms)]]
            best, _second, _ratio, verdict = aref.choose_chromosome(a, aref.sequence_bases(sizes, less), int(sizes[c]), MP, MR, 0)
            target = np.full(len(sizes), -1, np.int32)
            target[c] = q
            scores = aref.gap_scores(aref.table(P["pairs"], sizes, less, target, W)[0].reshape(-1, 2, 2), R)
            g, o, m, _runner_up, gap_verdict = aref.choose_gap(scores, MP)
            home = int(scores[k, "+-".index(o_c)])
            if verdict is None and best != q:
                word = "elsewhere"
            elif gap_verdict == "chromosome_only":
                word = "open"
            elif g != k:
                word = "move"
            elif gap_verdict == "orientation_open":
                word = "orientation_open"
            else:
                word = "flip" if o != o_c else "supported"
            out[c] = (word, g, o, int(m), home)
    return out, F


def test_the_planted_case_on_the_references_alone():
    P = eref.planted()
    calls, F = _leave_one_out(P, P["true_chroms"])
    assert F == 1940 and {v[0] for v in calls.values()} == {"supported"} and len(calls) == 40
    chroms = displaced_chroms(P["true_chroms"])
    assert [P["names"][chroms[q][j][0]] for q, _i, j, _t in DISPLACED] == ["scaf_3", "scaf_25", "scaf_33"]
    calls, F = _leave_one_out(P, chroms)
    assert F == 1675
    name = {n: s for s, n in enumerate(P["names"])}
    where = {s: (q, k, o) for q, chrom in enumerate(P["true_chroms"]) for k, (s, o) in enumerate(chrom)}
    for n, score, home in (("scaf_3", 290, 0), ("scaf_25", 86, 0), ("scaf_34", 241, 148)):
        word, g, o, m, h = calls[name[n]]
        assert (word, m, h) == ("move", score, home), (n, calls[name[n]])
        assert (g, o) == where[name[n]][1:]                                   # back to its true gap and sign
    assert sorted(P["names"][s] for s, v in calls.items() if v[0] == "move") == ["scaf_11", "scaf_25", "scaf_3", "scaf_33", "scaf_34"]
    assert [P["names"][s] for s, v in calls.items() if v[0] == "open"] == ["scaf_2"]
    assert calls[name["scaf_11"]][3] - calls[name["scaf_11"]][4] < 290 and calls[name["scaf_33"]][3] - calls[name["scaf_33"]][4] < 241 - 148


def displaced_files(tmp_path):
    P = eref.planted()
    text = lref.order_file_text(displaced_chroms(P["true_chroms"]), P["names"])
    cfg, order, save, _paths = anchor_cases._case_files(tmp_path, P["names"], P["sizes"], text, P["pairs"])
    return cfg, order, save


def check_displaced_outputs(moved_text, polished_text, report_text):
    """The outputs of the planted displaced case (also used by the GPU round trip)."""
    P = eref.planted()
    truth = lref.order_file_text(P["true_chroms"], P["names"])
    assert moved_text == truth and polished_text == truth
    rows = {r[0]: r for r in (line.split("\t") for line in report_text.splitlines() if not line.startswith("#"))}
    assert len(rows) == 40 and {len(r) for r in rows.values()} == {15}
    for n, home, score in (("scaf_3", "0", "290"), ("scaf_25", "0", "86"), ("scaf_34", "148", "241")):
        assert rows[n][14] == "move" and rows[n][7] == home and rows[n][11] == score and int(rows[n][13]) == int(score) - int(home)
    assert sorted(n for n, r in rows.items() if r[14] == "move") == ["scaf_11", "scaf_25", "scaf_3", "scaf_33", "scaf_34"]
    assert rows["scaf_2"][14] == "open" and sum(r[14] == "supported" for r in rows.values()) == 34


def _polish(cfg, order, out, more=(), context=None):
    from hic_genome_assembler_amd import polishOrder
    context = StandInContext() if context is None else context
    got = polishOrder.main(["-config", cfg, "-order", order, "-out", out] + list(more), context=context)
    assert context.calls[0] == "pairs_file" and context.calls.count("pairs_file") == 1
    assert context.calls[-1] == "pairs_drop" and context.store is None
    return got


def _summary(out):
    with open(os.path.join(out, "polish_summary.tsv")) as fh:
        head = dict(kv.split("=") for kv in fh.readline()[1:].rstrip("\n").split("\t"))
        columns = fh.readline()[1:].rstrip("\n").split("\t")
        rows = [line.rstrip("\n").split("\t") for line in fh if not line.startswith("#")]
    return head, columns, rows


def test_the_planted_displaced_case_returns_to_the_true_layout(tmp_path, capsys):
    from hic_genome_assembler_amd import supportSeats
    P = eref.planted()
    cfg, order, save = displaced_files(tmp_path)
    before = _read(order)
    ctx = StandInContext()
    moved, report, full = str(tmp_path / "moved.txt"), str(tmp_path / "seats.txt"), str(tmp_path / "full")
    stats, verdicts, moves = supportSeats.main(["-config", cfg, "-order", order, "-window", "5000", "-moved", moved, "-out", report,
                                                "-full", full], context=ctx)
    assert ctx.calls == ["pairs_file", "seats_resident", "pairs_drop"] and _read(order) == before
    where = {s: (q, k, o) for q, chrom in enumerate(P["true_chroms"]) for k, (s, o) in enumerate(chrom)}
    assert moves == {n: where[P["names"].index(n)] for n in ("scaf_3", "scaf_25", "scaf_34")}
    assert stats[:2] == (len(P["pairs"][0]),) * 2 and verdicts["scaf_2"] == "open"
    out = str(tmp_path / "polished")
    ctx = StandInContext()
    status, rounds, log = _polish(cfg, order, out, ["-moves", "flip,relocate", "-window", "5000"], context=ctx)
    check_displaced_outputs(_read(moved), _read(os.path.join(out, "orders.txt")), _read(report))
    assert (status, rounds) == ("converged", 1) and ctx.calls.count("seats_resident") == 2 and "anchor_resident" not in ctx.calls
    assert [row[:4] for row in log] == [(1, "relocate", 1, "scaf_3"), (1, "relocate", 2, "scaf_25"), (1, "relocate", 3, "scaf_34")]
    assert all(len(row) == 9 for row in log) and log[0][4:] == ("scaf_2", "scaf_4", where[2][2], 290, log[0][8])
    head, columns, rows = _summary(out)
    assert head["moves"] == "flip,relocate" and head["status"] == "converged" and columns[7] == "relocations" and len(columns) == 8
    assert [r[7] for r in rows] == ["1", "1", "1"] and sum(int(r[5]) for r in rows) == 1675 and sum(int(r[6]) for r in rows) == 1940
    assert "POLISH: converged after 1 round(s): 0 flip(s), 0 insertion(s), 3 relocation(s), facing links 1675 -> 1940" in capsys.readouterr().out
    # on the result every scaffold is supported
    report2 = str(tmp_path / "seats2.txt")
    supportSeats.main(["-config", cfg, "-order", moved, "-window", "5000", "-out", report2], context=StandInContext())
    assert _read(report2).count("\tsupported\n") == 40
    header = _read(report).splitlines()[0][1:].split("\t")
    assert header[:4] == ["window=5000", "reach=2", "minPairs=4", "minRatio=2"] and [kv.split("=")[0] for kv in header[4:]] == \
        ["lines", "used", "unknown_scaffold", "out_of_range", "seated", "middle", "trans", "same", "unlifted"]
    assert sum(int(kv.split("=")[1]) for kv in header[8:]) == len(P["pairs"][0])
    assert sorted(os.listdir(full)) == ["seats.chromosomes.tsv", "seats.gaps.tsv"]
    assert len(_read(os.path.join(full, "seats.chromosomes.tsv")).splitlines()) == 41
    assert os.listdir(save) == []


def test_without_relocate_nothing_is_moved_and_the_table_is_never_asked_for(tmp_path, capsys):
    cfg, order, _save = displaced_files(tmp_path)
    out = str(tmp_path / "polished")
    ctx = StandInContext()
    status, _rounds, log = _polish(cfg, order, out, ["-moves", "flip,place", "-window", "5000"], context=ctx)
    assert "seats_resident" not in ctx.calls and status in ("converged", "stalled") and not [row for row in log if row[1] != "flip"]
    polished = [line.split("\t")[0] for line in _read(os.path.join(out, "orders.txt")).splitlines()]
    assert polished == [line.split("\t")[0] for line in _read(order).splitlines()]          # the three lie where they lay
    head, columns, rows = _summary(out)
    assert len(columns) == 7 and all(len(r) == 7 for r in rows) and "relocation" not in capsys.readouterr().out


# ---- hand-built rounds -----------------------------------------------------------------------------------------------------------------
def test_a_relocate_round_that_does_not_raise_the_facing_links_is_undone_and_says_stalled(tmp_path):
    # window 2 on scaffolds of 10 bases: base 4 of b lies in its first half and in no end zone.  Six links of it with the
    # left end of d score the gap before d for b turned round, but a scaffold's middle adds nothing to the facing links.
    names, sizes = ["a", "b", "c", "d"], np.array([10, 10, 10, 10], dtype=np.int64)
    text = "### Chromosome grouping 1 ###\na\t+\nb\t+\nc\t+\nd\t+\n"
    pairs = _pairs([(1, 4, 3, 1)] * 6)
    cfg, order, _save, _paths = anchor_cases._case_files(tmp_path, names, sizes, text, pairs)
    out = str(tmp_path / "polished")
    ctx = StandInContext()
    status, rounds, log = _polish(cfg, order, out, ["-moves", "relocate", "-window", "2", "-reach", "1"], context=ctx)
    assert (status, rounds, log) == ("stalled", 0, []) and _read(os.path.join(out, "orders.txt")) == text
    assert ctx.calls.count("seats_resident") == 1 and ctx.calls.count("ends_resident") == 2
    head, _columns, rows = _summary(out)
    assert (head["status"], head["ended"]) == ("stalled", "nothing_left") and rows[0][7] == "0"


def test_the_round_limit_counts_relocate_rounds(tmp_path):
    cfg, order, _save = displaced_files(tmp_path)
    out = str(tmp_path / "polished")
    # a limit of one round: the one relocate round is applied, and nothing is left after it
    assert _polish(cfg, order, out, ["-moves", "flip,relocate", "-window", "5000", "-maxRounds", "1"])[:2] == ("converged", 1)
    # two scaffolds displaced in one chromosome need two rounds: a limit of one stops before the second
    P = eref.planted()
    chroms = [list(chrom) for chrom in P["true_chroms"]]
    chroms[0].insert(9, chroms[0].pop(2))
    chroms[0].insert(4, chroms[0].pop(11))
    cfg, order, _save, _paths = anchor_cases._case_files(tmp_path, P["names"], P["sizes"], lref.order_file_text(chroms, P["names"]), P["pairs"])
    out = str(tmp_path / "limited")
    status, rounds, log = _polish(cfg, order, out, ["-moves", "relocate", "-window", "5000", "-maxRounds", "1"])
    assert (status, rounds) == ("max_rounds", 1) and {row[0] for row in log} == {1} and _summary(out)[0]["ended"] == "round_limit"
    out = str(tmp_path / "free")
    status, rounds, log = _polish(cfg, order, out, ["-moves", "relocate", "-window", "5000"])
    assert status == "converged" and rounds >= 2 and _read(os.path.join(out, "orders.txt")) == lref.order_file_text(P["true_chroms"], P["names"])


def test_moved_order_text_keeps_every_other_byte(tmp_path):
    from hic_genome_assembler_amd.supportSeats import moved_order_text
    text = "### Chromosome grouping 1 ###\r\na\t+\r\nb\t+\tnote\r\nc\t-\r\n# remark\r\nd\t+\n### Chromosome grouping 2 ###\ne\t+\nf\t-\tx\ty\ng\t+"
    path = str(tmp_path / "o.txt")
    with open(path, "w", newline="") as fh:
        fh.write(text)
    # into the first gap, with the sign changed; into the last gap of a chromosome whose last line has no newline
    got = moved_order_text(path, {"c": ("a", "+"), "e": (("g", None), "-")})
    assert got == ("### Chromosome grouping 1 ###\r\nc\t+\r\na\t+\r\nb\t+\tnote\r\n# remark\r\nd\t+\n### Chromosome grouping 2 ###\n"
                   "f\t-\tx\ty\ng\t+\ne\t-")
    # the last line moved to the front: the file still ends without a newline, third columns travel with their line
    got = moved_order_text(path, {"g": ("e", "-"), "b": (("d", None), "+")})
    assert got == ("### Chromosome grouping 1 ###\r\na\t+\r\nc\t-\r\n# remark\r\nd\t+\nb\t+\tnote\r\n### Chromosome grouping 2 ###\n"
                   "g\t-\ne\t+\nf\t-\tx\ty")
    assert moved_order_text(path, {}) == text
    with open(path, "w", newline="") as fh:
        fh.write(text + "\n")
    assert moved_order_text(path, {"g": ("f", "+")}) == text.replace("f\t-\tx\ty\ng\t+", "g\t+\nf\t-\tx\ty") + "\n"


# ---- the nine verdicts --------------------------------------------------------------------------------------------------------------
V_NAMES = ["empty", "quiet", "stray", "single", "p0", "p1", "p2", "p3", "p4", "p5", "q0", "q1"]
V_SIZES = np.array([0, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10, 10], dtype=np.int64)
V_ORDER = ("### Chromosome grouping 1 ###\nempty\t+\nquiet\t+\np0\t+\np1\t+\np2\t+\np3\t+\np4\t+\np5\t+\nstray\t+\n"
           "### Chromosome grouping 2 ###\nq0\t+\nq1\t+\n### Chromosome grouping 3 ###\nsingle\t+\n")
EMPTY, QUIET, STRAY, SINGLE, P0, P1, P2, P3, P4, P5, Q0, Q1 = range(12)


def _verdict_rows():
    rows = [(STRAY, 5, Q0, 5)] * 9 + [(STRAY, 6, P5, 5)]                       # stray: Chr_2 stands out -> elsewhere
    rows += [(SINGLE, 1, Q1, 5)] * 2                                           # single: links, but no company -> alone
    rows += [(P0, 10, P1, 1)] * 3                                              # p0: three links, below minPairs 4 -> open
    rows += [(P1, 10, P2, 1)] * 5                                              # p1 (with the three above): home, as it lies -> supported
    rows += [(P2, 10, P4, 10)] * 8                                             # p2: its right half belongs behind p4 -> move
    rows += [(P3, 1, P4, 1)] * 6 + [(P3, 10, P2, 10)] * 6                      # p3: home, the other way round -> flip
    rows += [(P5, 1, P4, 10)] * 4 + [(P5, 10, P4, 10)] * 4                     # p5: home, both ways round the same -> orientation_open
    return rows


V_VERDICTS = {"empty": "NA", "quiet": "no_links", "stray": "elsewhere", "single": "alone", "p0": "open", "p1": "supported", "p2": "move",
              "p3": "flip", "p5": "orientation_open"}


def test_every_verdict_once_in_the_order_of_the_checks(tmp_path):
    from hic_genome_assembler_amd import supportSeats
    pairs = _pairs(_verdict_rows())
    cfg, order, _save, _paths = anchor_cases._case_files(tmp_path, V_NAMES, V_SIZES, V_ORDER, pairs)
    report = str(tmp_path / "seats.txt")
    _stats, verdicts, moves = supportSeats.main(["-config", cfg, "-order", order, "-window", "5", "-reach", "1", "-out", report],
                                                context=StandInContext())
    assert {n: verdicts[n] for n in V_VERDICTS} == V_VERDICTS, verdicts
    assert set(V_VERDICTS.values()) == {"NA", "no_links", "elsewhere", "alone", "open", "move", "orientation_open", "flip", "supported"}
    # p4 says move as well - between p2 and p3, turned, 14 against the 4 it has - and its gain of 10 beats p2's 3
    assert verdicts["p4"] == "move" and moves == {"p4": (0, 4, "-")}
    rows = {r[0]: r for r in (line.split("\t") for line in _read(report).splitlines() if not line.startswith("#"))}
    assert rows["empty"] == ["empty", "+", "0"] + ["NA"] * 12
    assert rows["quiet"][3:] == ["0", "0", "NA", "NA", "0", "NA", "NA", "NA", "0", "0", "0", "no_links"]
    assert rows["stray"][3:7] == ["10", "1", "2", "%.6g" % ((9 * 70) / (1 * 20))] and rows["single"][7:] == ["NA"] * 7 + ["alone"]
    assert rows["p2"][7:] == ["5", "p4", "p5", "-", "8", "6", "3", "move"]    # behind p3, turned, it would have 6
    assert rows["p3"][7:] == ["0", "p2", "p4", "-", "12", "0", "12", "flip"]
    assert rows["p5"][7:] == ["4", "p4", "stray", "+", "4", "4", "0", "orientation_open"]
    assert rows["p0"][7:] == ["3", "NA", "NA", "NA", "3", "0", "0", "open"]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_input_is_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import polishOrder, supportSeats, synth
    cfg, order, save = displaced_files(tmp_path)
    d = str(tmp_path)
    out = os.path.join(d, "seats.txt")
    ctx = StandInContext()

    def write(text, name):
        path = os.path.join(d, name)
        with open(path, "w") as fh:
            fh.write(text)
        return path

    def refused(word, more=(), config=cfg, order_file=order, tool=supportSeats):
        args = ["-config", config, "-out", out] + (["-order", order_file] if order_file else [])
        with pytest.raises(SystemExit) as exc:
            tool.main(args + list(more), context=ctx)
        assert word in str(exc.value.code) and str(exc.value.code).startswith("ERROR... ") and \
            str(exc.value.code).endswith(" Exiting..."), exc.value.code

    refused("window", ["-window", "0"])
    refused("reach", ["-reach", "0"])
    refused("reach", ["-reach", "65"])
    refused("minPairs", ["-minPairs", "-1"])
    refused("minRatio", ["-minRatio", "0.5"])
    refused("zz", order_file=write("### 1 ###\nscaf_2\t+\nzz\t+\n", "unknown.txt"))
    refused("twice", order_file=write("### 1 ###\nscaf_2\t+\n### 2 ###\nscaf_5\t+\nscaf_2\t-\n", "twice.txt"))
    refused("orientation", order_file=write("### 1 ###\nscaf_2\t+\nscaf_5\t?\n", "orient.txt"))
    refused("does not exist", order_file=os.path.join(d, "nothing_here"))
    refused("does not exist", order_file=None)
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    refused("validPairFile", config=synth.write_config(os.path.join(d, "c2.txt"), paths, save, os.path.join(d, "plots"), 100000))
    # 5,793 scaffolds in one chromosome: 5793 x (1 + 4 x 5793) counters pass 2^27, 5,792 do not
    n = 5793
    assert n * (1 + 4 * n) > 2 ** 27 >= (n - 1) * (1 + 4 * (n - 1))
    big = dict(paths, hicProScaffSizeFile=write("".join("s%d\t1\n" % k for k in range(n)), "big.sizes"))
    big_cfg = synth.write_config(os.path.join(d, "big.txt"), big, save, os.path.join(d, "plots"), 100000,
                                 extra={"validPairFile": os.path.join(d, "case.allValidPairs")})
    big_order = write("### 1 ###\n" + "".join("s%d\t+\n" % k for k in range(n)), "big.order")
    refused("%d counters" % (n * (1 + 4 * n)), config=big_cfg, order_file=big_order)
    # polishOrder makes the same check up front, and only when relocate is asked for
    out = os.path.join(d, "polished")
    refused("%d counters" % (n * (1 + 4 * n)), ["-moves", "flip,relocate"], config=big_cfg, order_file=big_order, tool=polishOrder)
    for moves in ("flip,swap", "", "place,", "relocate,"):
        refused("moves", ["-moves", moves], tool=polishOrder)
    assert ctx.calls == [] and not os.path.exists(out) and os.listdir(save) == [] and not os.path.exists(os.path.join(d, "seats.txt"))


# ---- header, binding, switch -----------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_export():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = re.sub(r"\s+", " ", fh.read())
    tables = "const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq"
    assert ("int hicmi_seats_resident(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, " + tables + ", int64_t window, "
            "uint64_t *table_out, uint64_t *counters5_out, int64_t *first_out, int64_t *n_table_out);") in text
    lib = _lib.load()
    assert len(_lib.SIGNATURES["hicmi_seats_resident"][1]) == 13 and hasattr(lib, "hicmi_seats_resident")
    assert re.search(r"int hicmi_seats_resident\(([^;]*)\);", text).group(1).count(",") + 1 == 13
    assert callable(_lib.Context.seats_resident) and lib.hicmi_abi_version() == 1
    assert set(_lib.SIGNATURES) == set(re.findall(r"\b(hicmi_[a-z0-9_]+)\(", text)) - {"hicmi_ctx"}
    for name in ("hicmi_seats_begin", "hicmi_seats_add_pairs", "hicmi_seats_finish", "hicmi_seats_file"):
        assert name not in text                                               # there is no such family


def test_binding_blocks_equal_the_reference():
    from hic_genome_assembler_amd import _lib
    for seed in SEEDS:
        sizes, tables, _pairs_, _window = _random_case(seed)
        first, n = _lib.seats_blocks(sizes, tables[0], len(tables[3]))
        want_first, want_n = ref.number_blocks(sizes, tables)
        assert first.dtype == np.int64 and first.tolist() == want_first.tolist() and n == want_n


def test_the_count_form_is_read_at_every_call_and_the_constants_are_named():
    with open(os.path.join(CSRC, "api_pairs.inc")) as fh:
        api = fh.read()
    assert 'getenv("HICMI_SEATS_PLAIN")' in api and api.count("seats_plain()") == 2          # a definition and one use
    call = api[api.index("int hicmi_seats_resident("):]
    assert "seats_plain()" in call and "pairs_resident_check(" in call and "seats_abandon(c)" in call
    for path in (os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc"))):
        with open(path) as fh:
            assert not [ln for ln in fh if "HICMI_SEATS_PLAIN" in ln and re.search(r"\bstatic\b[^;]*\bgetenv\(", ln)], path
    with open(os.path.join(CSRC, "hicmi_internal.h")) as fh:
        internal = fh.read()
    for name in ("SEATS_SLICE", "SEATS_SLOT_BITS", "SEATS_SLOTS", "SEATS_PROBES"):
        assert re.search(r"static constexpr int %s = " % name, internal), name
    with open(os.path.join(CSRC, "k_seats.hip")) as fh:
        kernel = fh.read()
    assert "static_assert((SEATS_SLOTS & (SEATS_SLOTS - 1)) == 0" in kernel and "static_assert(SEATS_SLICE % 256 == 0" in kernel
    assert "static_assert(SEATS_MAX_TABLE <= (int64_t)1 << 31" in kernel
    assert "k_seats_count<true>" in kernel and "k_seats_count<false>" in kernel and "__launch_bounds__(256)" in kernel
    assert "asm" not in re.sub(r"//[^\n]*", "", kernel)                       # plain C++: no inline assembly
    with open(os.path.join(CSRC, "seats.h")) as fh:
        includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", fh.read())
    assert includes == ['"anchor.h"']                                         # no GPU dependency
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    assert " seats.h " in make and " k_seats.hip " in make
    with open(os.path.join(ROOT, "README.md")) as fh:
        readme = fh.read()
    for word in ("supportSeats", "HICMI_SEATS_PLAIN", "k_seats.hip", "seats.h", "seatSupport.txt", "relocate"):
        assert word in readme, word
    # the call reads neither the contact matrix nor an open map, span, ends or anchor build
    for word in ("c->dC", "map_cells", "drop_matrix_state", "span_marks", "span_grid", "map_m", "ends_table", "ends_grid", "anchor_table",
                 "anchor_grid"):
        assert word not in call, word
