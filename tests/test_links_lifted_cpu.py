"""scaffoldLinks -rounds without a GPU: tests/links_lifted_reference.py against its own brute-force loop and,
on identity tables, against tests/links_reference.py; links_classify_lifted of csrc/links.h built as host code with the
sanitizers and compared line by line with the reference; the loop of rounds on a NumPy stand-in context - the planted assembly
ends in its three chromosomes -, ``-rounds 1`` byte for byte, the refusals and the plumbing.  Every comparison is of integers,
bit for bit."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import ends_reference as eref
import liftmap_reference as liftref
import links_lifted_reference as ref
import links_reference as lref
import pairs_reference as pref
import test_links_cpu as cpu

ROOT = cpu.ROOT
CSRC = cpu.CSRC
GAPS = (0, 1, 100)
WINDOWS = (1, 5, 10 ** 6)


def _same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def random_sequences(n_scaf, seed, drop=0.15):
    """Sequences of 1 to 3 scaffolds in a random order, half of the scaffolds reversed, some scaffolds in no sequence."""
    rng = np.random.default_rng(1000 + seed)
    pool = [int(s) for s in rng.permutation(n_scaf) if rng.random() >= drop]
    out = []
    while pool:
        k = int(rng.integers(1, 4))
        out.append([(s, "-" if rng.random() < .5 else "+") for s in pool[:k]])
        pool = pool[k:]
    return out or [[(0, "+")]]


def _random_case(seed):
    rng = np.random.default_rng(200 + seed)
    sizes = rng.integers(1, 40, int(rng.integers(3, 14))).astype(np.int64)
    gap = GAPS[seed % 3]
    tables = ref.tables_of(random_sequences(len(sizes), seed), sizes, gap)
    return sizes, tables, cpu.random_pairs(sizes, 300, seed), int(rng.integers(1, 30))


def zone_case(window, gap, seed=0):
    """The zone-edge scaffolds in sequences of 1 to 3, reversed ones among them and none dropped, with 2,000 pairs."""
    sizes = cpu.ZONE_SIZES
    tables = ref.tables_of(random_sequences(len(sizes), 50 + seed + gap, drop=0.0), sizes, gap)
    assert len(tables[3]) >= 3 and tables[2].any() and not tables[2].all()
    return sizes, tables, cpu.random_pairs(sizes, 2000, window + gap)


# ---- the reference against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", cpu.SEEDS)
def test_reference_rows_equal_the_brute_force_rows(seed):
    sizes, tables, pairs, window = _random_case(seed)
    got, want = ref.rows(pairs, sizes, tables, window), ref.brute_rows(pairs, sizes, tables, window)
    assert _same(got, want)
    lo, hi, counts, counters = got
    assert np.all(lo < hi) and int(counts.sum()) == int(counters[:2].sum()) and int(counters.sum()) == len(pairs[0])
    assert int(counts[:, :4].sum()) == int(counters[ref.LINKED])
    sa, pa, sb, pb = pairs
    assert _same(got, ref.rows((sb, pb, sa, pa), sizes, tables, window))                # mates swapped: the same rows


@pytest.mark.parametrize("gap", GAPS)
def test_reference_zone_edges(gap):
    for window in WINDOWS:
        sizes, tables, pairs = zone_case(window, gap)
        assert _same(ref.rows(pairs, sizes, tables, window), ref.brute_rows(pairs, sizes, tables, window))


def test_identity_tables_give_the_rows_of_the_scaffold_count():
    for seed in cpu.SEEDS:
        sizes, pairs, window = cpu._random_case(seed)
        lo, hi, counts, counters = ref.rows(pairs, sizes, liftref.identity(sizes), window)
        assert _same((lo, hi, counts, counters[:2]), lref.rows(pairs, sizes, window)) and counters[2:].tolist() == [0, 0]
    P = eref.planted(seed=7)
    kept = pref.keep(P["pairs"])
    got = ref.rows(kept, P["sizes"], ref.tables_of([[(s, "+")] for s in range(40)], P["sizes"], 100), 5000)
    assert _same(got[:3], lref.rows(kept, P["sizes"], 5000)[:3])


def test_zones_of_a_lifted_end_by_hand():
    # sequence 0 = B- (10 bases), gap 3, A+ (6 bases): 19 bases; sequence 1 = C+ (8 bases); D is dropped
    sizes = np.array([6, 10, 8, 5], dtype=np.int64)
    tables = ref.tables_of([[(1, "-"), (0, "+")], [(2, "+")]], sizes, 3)
    assert tables[0].tolist() == [0, 0, 1, -1] and tables[1].tolist() == [13, 0, 0, 0] and tables[3].tolist() == [19, 8]
    one = lambda sa, pa, sb, pb, w: ref.brute_classify(sizes, tables, w, sa, pa, sb, pb)       # noqa: E731
    # base 10 of B- is base 1 of the sequence: left; base 1 of C: left
    assert one(1, 10, 2, 1, 2) == (ref.LINKED, lref.key_of(0, 1, lref.LL))
    # base 6 of A+ is base 19 of the sequence: right; with C given first the key is the same and the first letter stays sequence 0's
    assert one(2, 8, 0, 6, 2) == (ref.LINKED, lref.key_of(0, 1, lref.RR)) and one(0, 6, 2, 1, 2) == (ref.LINKED, lref.key_of(0, 1, lref.RL))
    # base 1 of B- is base 10 of the sequence; window 9: the left zone ends at base 9, the right one begins at base 11
    assert one(1, 1, 2, 1, 9)[0] == ref.MIDDLE and one(1, 2, 2, 1, 9)[0] == ref.LINKED
    # the gap bases 11 .. 13 belong to the right zone at window 9: base 1 of A+ is base 14
    assert one(0, 1, 2, 1, 6) == (ref.LINKED, lref.key_of(0, 1, lref.RL)) and one(0, 1, 2, 1, 5)[0] == ref.MIDDLE
    assert one(0, 1, 1, 1, 5) == (ref.INSIDE, 0) and one(3, 1, 1, 1, 5) == (ref.UNLIFTED, 0) and one(0, 1, 3, 5, 5) == (ref.UNLIFTED, 0)


# ---- links_classify_lifted as host code under the sanitizers ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("links_lifted") / "links_lifted_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "links_lifted_host_check.cpp"), "-o", exe])

    def run(path, sizes, tables, window, pairs):
        lines = ["L %d %d %d" % (len(sizes), len(tables[3]), window)]
        lines += [" ".join(str(int(x)) for x in arr) for arr in (sizes, tables[0], tables[1], tables[2], tables[3])]
        lines += ["P %d" % len(pairs[0])] + ["%d %d %d %d" % row for row in zip(*(np.asarray(x).tolist() for x in pairs))]
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        # an ordinary child process, nothing preloaded
        done = subprocess.run([exe, path], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        return done.stdout.splitlines()
    return run


def _expected_lines(sizes, tables, window, pairs):
    out = ["pair %d %d" % ref.brute_classify(sizes, tables, window, *row) for row in zip(*(np.asarray(x).tolist() for x in pairs))]
    lo, hi, counts, counters = ref.rows(pairs, sizes, tables, window)
    out += ["counters %d %d %d %d" % tuple(int(c) for c in counters), "rows %d" % len(lo)]
    return out + ["row %d %d %d %d %d %d %d" % ((a, b) + tuple(row)) for a, b, row in zip(lo, hi, counts.tolist())]


@pytest.mark.parametrize("seed", cpu.SEEDS)
def test_native_lifted_keys_and_rows_under_the_sanitizers(seed, host_check, tmp_path):
    sizes, tables, pairs, window = _random_case(seed)
    assert host_check(str(tmp_path / "case.txt"), sizes, tables, window, pairs) == _expected_lines(sizes, tables, window, pairs)


@pytest.mark.parametrize("gap", GAPS)
@pytest.mark.parametrize("window", WINDOWS)
def test_native_lifted_zone_edges_under_the_sanitizers(window, gap, host_check, tmp_path):
    sizes, tables, pairs = zone_case(window, gap)
    assert host_check(str(tmp_path / "case.txt"), sizes, tables, window, pairs) == _expected_lines(sizes, tables, window, pairs)


def test_native_positions_and_offsets_above_2_to_the_32_every_scaffold_dropped_and_one_sequence(host_check, tmp_path):
    sizes = np.array([(1 << 40) + 1, 7, 1 << 33, 5], dtype=np.int64)
    tables = ref.tables_of([[(2, "-"), (0, "+")], [(1, "+"), (3, "-")]], sizes, 100)
    assert int(tables[1][0]) == (1 << 33) + 100 and int(tables[3][0]) > 1 << 40
    pairs = cpu._pairs([(0, 1 << 39, 1, 7), (1, 1, 2, 1 << 33), (3, 5, 0, (1 << 40) + 1), (0, 1, 2, 1), (2, (1 << 32) + 5, 3, 1),
                        (0, (1 << 40) - (1 << 32), 3, 2)])
    for window in ((1 << 32) + 5, 3, 1 << 41):
        got = host_check(str(tmp_path / "case.txt"), sizes, tables, window, pairs)
        assert got == _expected_lines(sizes, tables, window, pairs)
    dropped = (np.full(4, -1, np.int32), tables[1], tables[2], tables[3])
    assert host_check(str(tmp_path / "case.txt"), sizes, dropped, 3, pairs)[-2:] == ["counters 0 0 0 6", "rows 0"]
    one = ref.tables_of([[(0, "+"), (1, "-"), (2, "+"), (3, "+")]], sizes, 1)
    assert host_check(str(tmp_path / "case.txt"), sizes, one, 3, pairs)[-2:] == ["counters 0 0 6 0", "rows 0"]
    assert host_check(str(tmp_path / "case.txt"), sizes, one, 3, cpu._pairs([])) == ["counters 0 0 0 0", "rows 0"]


# ---- a path of sequences becomes a sequence -----------------------------------------------------------------------------------------
def test_paths_of_sequences_are_expanded_turned_and_numbered():
    from hic_genome_assembler_amd import scaffoldLinks as sl
    seqs = [[(0, "+")], [(1, "+"), (7, "-")], [(2, "-"), (5, "+"), (3, "+")], [(4, "+")], [(6, "+")]]
    # sequence 2 entered as -: 3- 5- 2+; then sequence 1 as +; the result ends at scaffold 7 and starts at 3: it stays
    after = sl.expand_paths(seqs, [[(2, "-"), (1, "+")]])
    assert after == [[(0, "+")], [(3, "-"), (5, "-"), (2, "+"), (1, "+"), (7, "-")], [(4, "+")], [(6, "+")]]
    # a path that would start at its terminal scaffold of higher index is turned
    after = sl.expand_paths(seqs, [[(4, "+"), (0, "-")], [(1, "-"), (3, "+")]])
    assert after == [[(0, "+"), (6, "-")], [(2, "-"), (5, "+"), (3, "+")], [(4, "-"), (1, "+"), (7, "-")]]
    assert sl.expand_paths(seqs, []) == seqs
    # the layout: offsets from 0 with the gap between neighbours, as the reference lays it out
    sizes = np.arange(10, 18, dtype=np.int64)
    for gap in GAPS:
        assert _same(sl.sequence_tables(after, sizes, gap), ref.tables_of(after, sizes, gap))
    assert sl.sequence_tables(after, sizes, 100)[3].tolist() == [10 + 16 + 100, 12 + 15 + 13 + 200, 14 + 11 + 17 + 200]
    assert _same(sl.sequence_tables([[(s, "+")] for s in range(8)], sizes, 100), liftref.identity(sizes))
    assert sl.next_window(5000, 1.0) == 5000 and sl.next_window(5000, 2.0) == 10000 and sl.next_window(3, 1.5) == 4
    assert sl.layout_paths(after, sizes) == [after[2], after[1], after[0]]


# ---- the loop on the stand-in ------------------------------------------------------------------------------------------------------------
def _table(path):
    return cpu._table(path)


def _rounds(out):
    lines = cpu._read(os.path.join(out, "rounds.tsv")).splitlines()
    assert lines[0] == "#round\twindow\tsequences_in\trows\tlinked\tmiddle\tinside\tunlifted\tjoins\tcycles_cut\tsequences_out\tpaths\tsingles"
    assert lines[-1].startswith("#ended=")
    return [[int(x) for x in line.split("\t")] for line in lines[1:-1]], lines[-1][len("#ended="):]


def _order_paths(path, names):
    from hic_genome_assembler_amd.assembledMap import read_order_file
    index = {n: s for s, n in enumerate(names)}
    return [[(index[n], o) for n, o in group] for group in read_order_file(path)]


def check_final_order(path, P):
    """final.order holds all 40 scaffolds in 3 paths, each a true chromosome or its reverse complement."""
    flip = {"+": "-", "-": "+"}
    paths = _order_paths(path, P["names"])
    assert len(paths) == 3 and sorted(s for p in paths for s, _o in p) == list(range(40))
    left = [list(c) for c in P["true_chroms"]]
    for p in paths:
        back = [(s, flip[o]) for s, o in reversed(p)]
        match = [c for c in left if c in (p, back)]
        assert len(match) == 1, p
        left.remove(match[0])
    assert left == []


@functools.lru_cache(maxsize=None)
def planted_round2_tables():
    """(P, kept pairs, the eight sequences round 1 leaves on the planted pairs, their tables at gap 100): read only."""
    from hic_genome_assembler_amd import scaffoldLinks as sl
    P = eref.planted(seed=7)
    kept = pref.keep(P["pairs"])
    lo, hi, counts, _c = lref.rows(kept, P["sizes"], eref.PLANTED_WINDOW)
    paths = sl.decide(lo, hi, counts, P["sizes"], eref.PLANTED_MIN_PAIRS, 2.0, 0)[3]
    sequences = sl.expand_paths([[(s, "+")] for s in range(40)], paths)
    tables = ref.tables_of(sequences, P["sizes"], 100)
    for a in kept + tables:
        a.setflags(write=False)
    return P, kept, sequences, tables


@pytest.mark.parametrize("growth", [1, 2])
def test_planted_assembly_ends_in_its_three_chromosomes(growth, tmp_path, capsys):
    from hic_genome_assembler_amd import scaffoldLinks
    P, cfg, order, _save = cpu.planted_files(tmp_path)
    out = str(tmp_path / "links")
    ctx = ref.StandInContext()
    more = ["-growth", str(growth)] if growth != 1 else []
    _stats, joins, paths = scaffoldLinks.main(["-config", cfg, "-out", out, "-window", "5000", "-rounds", "5", "-order", order] + more,
                                              context=ctx)
    assert ctx.calls == ["pairs_file", "links_resident", "links_lifted", "links_lifted", "pairs_drop"] and ctx.store is None
    assert len(joins) == 32 and len(paths) == 8
    rounds, ended = _rounds(out)
    assert ended == "nothing_left" and [r[0] for r in rounds] == [1, 2, 3]
    assert [r[1] for r in rounds] == [5000, 5000 * growth, 5000 * growth ** 2]
    # round, sequences in, joins, cycles cut, sequences out, paths, singles
    assert [(r[2], r[8], r[9], r[10], r[11], r[12]) for r in rounds] == [(40, 32, 0, 8, 8, 0), (8, 5, 0, 3, 3, 0), (3, 0, 0, 3, 3, 0)]
    assert all(sum(r[4:8]) == 17334 for r in rounds) and rounds[0][6:8] == [0, 0]
    # what the prototype of the issue saw in round 2
    assert rounds[1][3] == 28 and rounds[1][6] == 12186 and rounds[1][7] == 0
    assert rounds[1][4:6] == ([240, 4908] if growth == 1 else [536, 4612])
    check_final_order(os.path.join(out, "final.order"), P)
    assert cpu._read(os.path.join(out, "final.order")) == cpu._read(os.path.join(out, "round2", "paths.order")) \
        == cpu._read(os.path.join(out, "round3", "paths.order"))
    assert sorted(os.listdir(out)) == ["ends.tsv", "final.order", "junctions.tsv", "links.tsv", "links_summary.tsv", "paths.order",
                                       "round2", "round3", "rounds.tsv"]
    for r in ("round2", "round3"):
        assert sorted(os.listdir(os.path.join(out, r))) == ["ends.tsv", "links.tsv", "paths.order", "sequences.tsv"]
    # round 2's sequences are round 1's paths, numbered by their first scaffold, and its tables are the reference's
    _P, _kept, sequences, tables = planted_round2_tables()
    seq_rows = _table(os.path.join(out, "round2", "sequences.tsv"))
    assert [r[0] for r in seq_rows] == ["seq_%d" % k for k in range(1, 9)]
    assert [r[3] for r in seq_rows] == [",".join(P["names"][s] + o for s, o in m) for m in sequences]
    assert [int(r[2]) for r in seq_rows] == tables[3].tolist() and [int(r[1]) for r in seq_rows] == [len(m) for m in sequences]
    assert [m[0][0] for m in sequences] == sorted(m[0][0] for m in sequences) and all(m[0][0] < m[-1][0] for m in sequences)
    assert _order_paths(os.path.join(out, "paths.order"), P["names"]) == sorted(sequences, key=lambda m: (-sum(int(P["sizes"][s]) for s, _o in m), m[0][0]))
    links = _table(os.path.join(out, "round2", "links.tsv"))
    assert len(links) == 28 and all(r[0].startswith("seq_") and r[1].startswith("seq_") for r in links)
    ends = _table(os.path.join(out, "round2", "ends.tsv"))
    assert len(ends) == 16 and sum(r[11] == "joined" for r in ends) == 10 and {len(r) for r in ends} == {12}
    assert sum(r[11] == "joined" for r in _table(os.path.join(out, "round3", "ends.tsv"))) == 0
    printed = capsys.readouterr().out.splitlines()
    assert printed[0] == "LINKS: scaffolds 40, pairs kept 17334, rows %d, joins 32, paths 8" % rounds[0][3]
    assert printed[1] == "LINKS round 2: window %d, sequences 8, rows 28, joins 5, sequences out 3" % (5000 * growth)
    assert printed[2].startswith("LINKS round 3: window %d, sequences 3, " % (5000 * growth ** 2)) and printed[2].endswith("joins 0, sequences out 3")
    assert printed[3:] == ["LINKS: 3 rounds, ended nothing_left, paths 3, singles 0"]


def test_the_round_limit_ends_the_loop_and_a_round_without_a_join_ends_it_first(tmp_path):
    from hic_genome_assembler_amd import scaffoldLinks
    P, cfg, _order, _save = cpu.planted_files(tmp_path)
    out = str(tmp_path / "two")
    ctx = ref.StandInContext()
    scaffoldLinks.main(["-config", cfg, "-out", out, "-window", "5000", "-rounds", "2"], context=ctx)
    rounds, ended = _rounds(out)
    assert ended == "round_limit" and len(rounds) == 2 and ctx.calls == ["pairs_file", "links_resident", "links_lifted", "pairs_drop"]
    check_final_order(os.path.join(out, "final.order"), P)
    assert not os.path.exists(os.path.join(out, "round3")) and not os.path.exists(os.path.join(out, "junctions.tsv"))
    # -minPairs above every count: round 1 joins nothing, no later round is counted, and the last layout is empty
    out = str(tmp_path / "none")
    ctx = ref.StandInContext()
    scaffoldLinks.main(["-config", cfg, "-out", out, "-window", "5000", "-rounds", "3", "-minPairs", "100000"], context=ctx)
    rounds, ended = _rounds(out)
    assert ended == "nothing_left" and [(r[0], r[8], r[10], r[11], r[12]) for r in rounds] == [(1, 0, 40, 0, 40)]
    assert ctx.calls == ["pairs_file", "links_resident", "pairs_drop"] and cpu._read(os.path.join(out, "final.order")) == ""
    assert not os.path.exists(os.path.join(out, "round2"))


def test_rounds_1_is_the_run_without_the_flag_byte_for_byte(tmp_path, capsys):
    from hic_genome_assembler_amd import scaffoldLinks
    _P, cfg, order, _save = cpu.planted_files(tmp_path)
    files = ["ends.tsv", "junctions.tsv", "links.tsv", "links_summary.tsv", "paths.order"]
    made, printed = {}, {}
    for name, more in (("plain", []), ("one", ["-rounds", "1"]), ("grown", ["-rounds", "1", "-growth", "3", "-gap", "0"])):
        out = str(tmp_path / name)
        ctx = ref.StandInContext()
        made[name] = scaffoldLinks.main(["-config", cfg, "-out", out, "-window", "5000", "-order", order] + more, context=ctx)
        assert ctx.calls == ["pairs_file", "links_resident", "pairs_drop"]                  # no links_lifted call
        assert sorted(os.listdir(out)) == files                                             # no round2/, rounds.tsv or final.order
        made[name] = (made[name], [cpu._read(os.path.join(out, fn)) for fn in files])
        printed[name] = capsys.readouterr().out
    assert made["plain"] == made["one"] == made["grown"] and printed["plain"] == printed["one"] == printed["grown"]
    assert printed["plain"].count("\n") == 1


def test_bad_rounds_growth_and_gap_are_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import scaffoldLinks
    _P, cfg, _order, save = cpu.planted_files(tmp_path)
    out = str(tmp_path / "links")
    ctx = ref.StandInContext()
    for word, more in (("rounds", ["-rounds", "0"]), ("rounds", ["-rounds", "-2"]), ("growth", ["-growth", "0.99"]),
                       ("growth", ["-growth", "nan"]), ("gap", ["-gap", "-1"]), ("growth", ["-rounds", "1", "-growth", "0.5"])):
        with pytest.raises(SystemExit) as exc:
            scaffoldLinks.main(["-config", cfg, "-out", out] + more, context=ctx)
        assert word in str(exc.value.code) and str(exc.value.code).startswith("ERROR... ") and str(exc.value.code).endswith(" Exiting...")
    assert ctx.calls == [] and not os.path.exists(out) and os.listdir(save) == []

    class Refusing(ref.StandInContext):
        def links_lifted(self, *args):
            from hic_genome_assembler_amd import _lib
            raise _lib.HicmiError("libhicmi error -1: the tables are refused")

    ctx = Refusing()
    with pytest.raises(SystemExit) as exc:
        scaffoldLinks.main(["-config", cfg, "-out", out, "-window", "5000", "-rounds", "2"], context=ctx)
    assert "the tables are refused" in str(exc.value.code) and ctx.calls == ["pairs_file", "links_resident", "pairs_drop"]
    assert not os.path.exists(out)


# ---- header, binding, Makefile -----------------------------------------------------------------------------------------------------------
def test_header_binding_and_makefile_name_the_call_and_its_file():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = re.sub(r"\s+", " ", fh.read())
    assert ("int hicmi_links_lifted(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq, "
            "const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq, int64_t window, "
            "int64_t *n_rows_out, uint64_t *counters4_out);") in text
    assert len(_lib.SIGNATURES["hicmi_links_lifted"][1]) == 11 and hasattr(_lib.load(), "hicmi_links_lifted")
    assert callable(_lib.Context.links_lifted)
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    assert re.search(r"^api\.o:.*\bapi_links\.inc\b", make, re.M) and re.search(r"^api\.o:.*\bapi_pairs\.inc\b", make, re.M)
    with open(os.path.join(CSRC, "api.hip")) as fh:
        api = fh.read()
    assert api.index('#include "api_pairs.inc"') < api.index('#include "api_links.inc"')
    with open(os.path.join(CSRC, "api_links.inc")) as fh:
        call = fh.read()
    # the switch is read at every call, the store is checked and only read, and no matrix state or open build is touched
    assert call.count("links_plain()") == 1 and "getenv" not in call and "pairs_resident_check(" in call and "lift_check(" in call
    assert "links_capacity(c->pairs_len, n_seq" in call and "launch_links_compact(" in call and "links_sort_records(" in call
    for word in ("c->dC", "map_cells", "drop_matrix_state", "span_marks", "span_grid", "map_m", "ends_table", "ends_grid", "anchor_table",
                 "anchor_grid", "seats_table"):
        assert word not in call, word
    with open(os.path.join(CSRC, "k_links.hip")) as fh:
        kernel = fh.read()
    assert "k_links_count_lifted<true>" in kernel and "k_links_count_lifted<false>" in kernel and "links_classify_lifted(" in kernel
    with open(os.path.join(CSRC, "links.h")) as fh:
        shared = fh.read()
    assert "LIFT_HD int links_classify_lifted(const LiftTables& L, const int64_t* seq_size," in shared
    assert re.findall(r"#include\s+([<\"][^>\"]+[>\"])", shared) == ['"ends.h"']
    with open(os.path.join(ROOT, "README.md")) as fh:
        readme = fh.read()
    for word in ("-rounds", "-growth", "hicmi_links_lifted", "rounds.tsv", "final.order", "sequences.tsv"):
        assert word in readme, word
