"""supportEnds without a GPU: tests/ends_reference.py against its own brute-force table and hand-worked
cases, csrc/ends.h built as host code with the sanitizers and compared line by line with the reference, the declarations,
the report and the refusals of the command line on a fake context that answers from the reference, and the planted
flips.  Every comparison is exact."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import buildmap_reference as bref
import ends_reference as ref
import liftmap_reference as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")

# six scaffolds a .. f; Chr_1 = c-, b-, a+ (b has one base), Chr_2 = d+, f+ (f has no base), e is not placed
NAMES = ["a", "b", "c", "d", "e", "f"]
SIZES = np.array([5, 1, 7, 3, 4, 0], dtype=np.int64)
CHROMS = [[(2, "-"), (1, "-"), (0, "+")], [(3, "+"), (5, "+")]]
A, B, C, D, E, F = range(6)


def _pairs(rows):
    sa, pa, sb, pb = zip(*rows)
    return (np.array(sa, np.int32), np.array(pa, np.int64), np.array(sb, np.int32), np.array(pb, np.int64))


# ---- the reference against itself and hand-worked cases ----------------------------------------------------------------------
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", [0, 1, 100])
def test_ranks_against_hand_worked_cases(gap, drop):
    tables = lref.layout(CHROMS, SIZES, gap, drop_unplaced=drop)
    rank, seq_first, n = ref.number_ranks(SIZES, tables)
    # c, b, a in Chr_1; d alone in Chr_2 (f has no base); e a sequence of its own unless it is dropped
    assert rank.tolist() == [2, 1, 0, 3, -1 if drop else 4, -1] and n == (4 if drop else 5)
    assert seq_first.tolist() == ([0, 3, 4] if drop else [0, 3, 4, 5])


def test_zones_at_lengths_1_2_3_and_windows_1_half_and_beyond():
    sizes = np.array([1, 2, 3, 7, 7], dtype=np.int64)
    tables = lref.layout([[(0, "+"), (1, "+"), (2, "+"), (3, "+"), (4, "-")]], sizes, 0)
    L, R, M = ref.LEFT, ref.RIGHT, ref.MID

    def zones_of(s, window):
        n = int(sizes[s])
        return ref.zones([s] * n, list(range(1, n + 1)), sizes, tables, window).tolist()

    for W in (1, 2, 10 ** 9):
        assert zones_of(0, W) == [L]                                   # one base: all LEFT
        assert zones_of(1, W) == [L, R]
    assert zones_of(2, 1) == [L, M, R] and zones_of(2, 2) == [L, L, R] and zones_of(2, 100) == [L, L, R]
    assert zones_of(3, 1) == [L, M, M, M, M, M, R]
    assert zones_of(3, 3) == [L, L, L, M, R, R, R]                     # W = L / 2: the middle base is left over
    assert zones_of(3, 4) == [L, L, L, L, R, R, R] and zones_of(3, 1000) == [L, L, L, L, R, R, R]
    # the reversed one: base 7 lies first
    assert zones_of(4, 1) == [R, M, M, M, M, M, L] and zones_of(4, 3) == [R, R, R, M, L, L, L]
    assert zones_of(4, 1000) == [R, R, R, L, L, L, L]
    assert [ref.zone_sizes(n, w) for n, w in ((1, 5), (2, 5), (3, 1), (3, 5), (7, 3), (7, 9))] == [(1, 0), (1, 1), (1, 1), (2, 1), (3, 3), (4, 3)]


@pytest.mark.parametrize("gap", [0, 1, 100])
def test_a_pair_across_a_junction_lands_in_facing_and_after_a_flip_where_the_definitions_say(gap):
    # base 1 of c is the last base of c- as it lies, base 1 of a the first one of a+
    pair = _pairs([(C, 1, A, 1)])
    swapped = _pairs([(A, 1, C, 1)])
    for chrom, d in (([(C, "-"), (A, "+")], 1), ([(C, "-"), (B, "-"), (A, "+")], 2)):
        for oc, oa, where in (("-", "+", ref.RL), ("+", "+", ref.LL), ("-", "-", ref.RR), ("+", "-", ref.LR)):
            lying = [(s, {C: oc, A: oa}.get(s, o)) for s, o in chrom]
            tables = lref.layout([lying, [(D, "+"), (F, "+")]], SIZES, gap)
            for p in (pair, swapped):
                T, counters = ref.table(p, SIZES, tables, 2, 2)
                want = np.zeros_like(T)
                want[0, d - 1, where] = 1
                assert T.tobytes() == want.tobytes() and counters.tolist() == [1, 0, 0, 0, 0, 0]
            if d == 1:
                figures = ref.junction_figures(T, 0)
                assert figures == tuple(int(k == where) for k in (ref.RL, ref.LL, ref.RR, ref.LR))
                assert ref.junction_verdict(figures, 1) == {ref.RL: "held", ref.LL: "flip_left", ref.RR: "flip_right", ref.LR: "flip_both"}[where]
                assert ref.junction_verdict(figures, 2) == "open"
            # the scaffold figures: c has the rank 0, a the rank d
            _rank, seq_first, _n = ref.number_ranks(SIZES, tables)
            c_fig, a_fig = ref.scaffold_figures(T, seq_first, 0)[:2], ref.scaffold_figures(T, seq_first, d)[:2]
            assert c_fig == {ref.RL: (1, 0), ref.LL: (0, 1)}.get(where, (0, 0))
            assert a_fig == {ref.RL: (1, 0), ref.RR: (0, 1)}.get(where, (0, 0))


def test_kinds_in_the_order_of_the_definitions_and_the_table_whatever_the_gap():
    ends = [(s, p) for s in range(5) for p in range(1, int(SIZES[s]) + 1)]
    pairs = _pairs([a + b for a in ends for b in ends])                    # every end against every end
    seen = None
    for gap in (0, 1, 100):
        tables = lref.layout(CHROMS, SIZES, gap, drop_unplaced=True)
        got = [ref.table(pairs, SIZES, tables, W, R) for W in (1, 2, 3, 100) for R in (1, 2)]
        blob = b"".join(T.tobytes() + c.tobytes() for T, c in got)
        assert seen is None or blob == seen
        seen = blob
    # W = 1, R = 1: e is dropped (every pair with an end on it is unlifted, before anything else is asked)
    T, counters = ref.table(pairs, SIZES, tables, 1, 1)
    n_e, n_all = 4, len(ends)
    assert counters[ref.UNLIFTED] == n_all * n_all - (n_all - n_e) ** 2
    assert counters[ref.TRANS] == 2 * 13 * 3                               # Chr_1 has 13 bases, d has 3
    assert counters[ref.SAME] == 25 + 1 + 49 + 9
    assert counters[ref.TOO_FAR] == 2 * 7 * 5                              # c and a are two ranks apart
    # c - b and b - a: b's one base is LEFT, c has the zone bases 7 (LEFT) and 1 (RIGHT), a the bases 1 (LEFT) and 5 (RIGHT)
    assert counters[ref.LINKED] == 2 * (2 + 2) and counters[ref.MIDDLE] == 2 * (7 + 5) - 8
    want = np.zeros((4, 1, 4), np.uint64)
    want[0, 0, ref.LL] = want[0, 0, ref.RL] = want[1, 0, ref.LL] = want[1, 0, ref.LR] = 2
    assert T.tobytes() == want.tobytes() and int(counters.sum()) == len(pairs[0])


def _random_case(seed):
    rng = np.random.default_rng(seed)
    S = int(rng.integers(4, 12))
    sizes = rng.integers(0, 30, S).astype(np.int64)
    order = rng.permutation(S).tolist()
    n_placed = int(rng.integers(3, S + 1))
    cut = int(rng.integers(1, n_placed))
    chroms = [[(s, "+-"[int(rng.integers(0, 2))]) for s in part] for part in (order[:cut], order[cut:n_placed])]
    tables = lref.layout(chroms, sizes, int(rng.choice([0, 1, 100])), drop_unplaced=bool(rng.integers(0, 2)))
    have = np.flatnonzero(sizes > 0)
    n = 300
    sa, sb = rng.choice(have, n), rng.choice(have, n)
    near = rng.random(n) < 0.2
    sb[near] = sa[near]
    pa = 1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64)
    return sizes, tables, (sa.astype(np.int32), pa, sb.astype(np.int32), pb), int(rng.choice([1, 4, 9, 1000])), int(rng.choice([1, 2, 3, 64]))


@pytest.mark.parametrize("seed", range(12))
def test_reference_table_equals_the_brute_force_table(seed):
    sizes, tables, pairs, window, reach = _random_case(seed)
    T, counters = ref.table(pairs, sizes, tables, window, reach)
    bT, bc = ref.brute_table(pairs, sizes, tables, window, reach)
    assert T.dtype == np.uint64 and T.shape == bT.shape and T.tobytes() == bT.tobytes() and counters.tolist() == bc.tolist()
    _rank, seq_first, n = ref.number_ranks(sizes, tables)
    assert int(counters.sum()) == len(pairs[0]) and int(T.sum()) == int(counters[ref.LINKED]) and T.shape == (n, reach, 4)
    assert not ref.outside(T, seq_first).any()


def test_the_random_cases_hold_every_kind_of_pair():
    total = np.zeros(6, np.uint64)
    for seed in range(12):
        sizes, tables, pairs, window, reach = _random_case(seed)
        total += ref.table(pairs, sizes, tables, window, reach)[1]
    assert (total > 20).all(), total


def test_verdicts():
    assert [ref.scaffold_verdict(*x) for x in ((3, 1, False, 4), (1, 3, False, 4), (2, 2, False, 4), (2, 1, False, 4), (0, 0, False, 0), (9, 0, True, 0))] \
        == ["supported", "flip", "open", "open", "open", "NA"]
    assert [ref.junction_verdict(f, m) for f, m in (((3, 1, 0, 0), 4), ((1, 3, 0, 0), 4), ((0, 1, 3, 0), 4), ((0, 0, 1, 3), 4), ((2, 2, 1, 0), 4),
                                                    ((2, 1, 0, 0), 4), ((0, 0, 0, 0), 0), ((1, 0, 0, 0), 0))] \
        == ["held", "flip_left", "flip_right", "flip_both", "open", "open", "open", "held"]


# ---- ends.h as host code under the sanitizers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ends") / "ends_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "ends_host_check.cpp"), "-o", exe])

    def run(path, sizes, tables, window, reach, pairs, print_table=True):
        seq, off, rev, seq_sizes = tables
        lines = ["T %d %d %d %d %d" % (len(sizes), len(seq_sizes), window, reach, print_table)]
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


def _expected_lines(sizes, tables, window, reach, pairs):
    rank, seq_first, n = ref.number_ranks(sizes, tables)
    kind, index = ref.classify(pairs, sizes, tables, window, reach)
    T, counters = ref.table(pairs, sizes, tables, window, reach)
    out = ["check 0 ", "placed %d" % n] + ["rank %d" % r for r in rank] + ["seq %d" % r for r in seq_first]
    out += ["pair %d %d" % ki for ki in zip(kind.tolist(), index.tolist())]
    return out + ["counters " + " ".join(str(c) for c in counters.tolist())] + ["t %d" % c for c in T.reshape(-1).tolist()]


@pytest.mark.parametrize("seed", range(12))
def test_native_ranks_kinds_and_table_under_the_sanitizers(seed, host_check, tmp_path):
    sizes, tables, pairs, window, reach = _random_case(seed)
    assert host_check(str(tmp_path / "case.txt"), sizes, tables, window, reach, pairs) == _expected_lines(sizes, tables, window, reach, pairs)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", [0, 1, 100])
def test_native_hand_worked_assembly_under_the_sanitizers(gap, drop, host_check, tmp_path):
    tables = lref.layout(CHROMS, SIZES, gap, drop_unplaced=drop)
    ends = [(s, p) for s in range(5) for p in range(1, int(SIZES[s]) + 1)]
    pairs = _pairs([a + b for a in ends for b in ends])
    for window in (1, 2, 3, 100):
        for reach in (1, 2, 64):
            got = host_check(str(tmp_path / "case.txt"), SIZES, tables, window, reach, pairs)
            assert got == _expected_lines(SIZES, tables, window, reach, pairs)
    assert got[1] == ("placed 4" if drop else "placed 5")


def test_native_positions_above_2_to_the_32_under_the_sanitizers(host_check, tmp_path):
    L = 2 ** 33
    big = 2 ** 62 - 5                                                   # next to the largest size an offset can carry
    sizes = np.array([L, L + 1, L, 5, big], dtype=np.int64)
    tables = lref.layout([[(0, "+"), (1, "-"), (2, "+")], [(4, "-")]], sizes, 100)
    for window in (1, 2 ** 20, 2 ** 32, 2 ** 32 + 1, 2 ** 62):
        mid = L // 2
        edge = [1, 2, window, window + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, mid, mid + 1, mid + 2, L - window, L - window + 1, L - 1, L]
        ends = [(s, p) for s in range(3) for p in edge if 1 <= p <= sizes[s]] + [(1, L + 1), (3, 1), (3, 5), (4, 1), (4, big), (4, big // 2), (4, big - big // 2)]
        pairs = _pairs([a + b for a in ends for b in ends])
        for reach in (1, 2):
            got = host_check(str(tmp_path / "case.txt"), sizes, tables, window, reach, pairs)
            assert got == _expected_lines(sizes, tables, window, reach, pairs)
    assert ref.zones([4, 4, 4], [1, big // 2 + 1, big], sizes, tables, 2 ** 62).tolist() == [ref.RIGHT, ref.LEFT, ref.LEFT]


def test_native_table_limit_from_both_sides_under_the_sanitizers(host_check, tmp_path):
    none = _pairs([(0, 1, 0, 1)])
    for reach, most in ((64, 2 ** 19), (48, 2 ** 25 // 48)):
        assert ref.fits(most, reach) and not ref.fits(most + 1, reach)
        for n, fit in ((most, True), (most + 1, False)):
            sizes = np.ones(n, np.int64)
            tables = lref.layout([[(s, "+") for s in range(n)]], sizes, 0)
            got = host_check(str(tmp_path / "case.txt"), sizes, tables, 1, reach, none, print_table=False)
            if fit:
                assert got[:2] == ["check 0 ", "placed %d" % n] and got[2:n + 2] == ["rank %d" % r for r in range(n)]
                assert got[n + 2:] == ["seq 0", "seq %d" % n, "pair %d -1" % ref.SAME, "counters 0 0 1 0 0 0"]
            else:
                assert got == ["check 0 ", "placed -1"]


# ---- header, binding, switch ---------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_exports():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = re.sub(r"\s+", " ", fh.read())
    tables = "const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq"
    assert ("int hicmi_ends_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, " + tables + ", int64_t window, "
            "int64_t reach, int32_t *rank_out, int64_t *n_placed_out);") in text
    assert ("int hicmi_ends_add_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b, "
            "const int64_t *pos_b, int64_t n);") in text
    assert "int hicmi_ends_finish(hicmi_ctx *ctx, uint64_t *table_out, uint64_t *counters6_out);" in text
    assert ("int hicmi_ends_file(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names, "
            "const int64_t *scaf_size, " + tables + ", int64_t window, int64_t reach, hicmi_ctx *ctx, int threads, int64_t *stats5, "
            "uint64_t *table_out, uint64_t *counters6_out, int32_t *rank_out, int64_t *n_placed_out);") in text
    lib = _lib.load()
    for name, n_args in {"hicmi_ends_begin": 12, "hicmi_ends_add_pairs": 6, "hicmi_ends_finish": 3, "hicmi_ends_file": 19}.items():
        assert len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
        declared = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        assert declared.count(",") + 1 == n_args
    for method in ("ends_begin", "ends_add_pairs", "ends_finish"):
        assert callable(getattr(_lib.Context, method))
    assert callable(_lib.ends_file) and lib.hicmi_abi_version() == 1
    assert set(_lib.SIGNATURES) == set(re.findall(r"\b(hicmi_[a-z0-9_]+)\(", text)) - {"hicmi_ctx"}


def test_the_count_form_is_read_at_every_call_and_the_constants_are_named():
    with open(os.path.join(CSRC, "api.hip")) as fh:
        api = fh.read()
    assert 'getenv("HICMI_ENDS_PLAIN")' in api and api.count("ends_plain()") == 3          # a definition and two uses
    for path in (os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))):
        with open(path) as fh:
            assert not [ln for ln in fh if "HICMI_ENDS_PLAIN" in ln and re.search(r"\bstatic\b[^;]*\bgetenv\(", ln)], path
    with open(os.path.join(CSRC, "hicmi_internal.h")) as fh:
        internal = fh.read()
    for name in ("ENDS_SLICE", "ENDS_SLOT_BITS", "ENDS_SLOTS", "ENDS_PROBES"):
        assert re.search(r"static constexpr int %s = " % name, internal), name
    with open(os.path.join(CSRC, "k_ends.hip")) as fh:
        kernel = fh.read()
    assert "static_assert((ENDS_SLOTS & (ENDS_SLOTS - 1)) == 0" in kernel and "static_assert(ENDS_SLICE % 256 == 0" in kernel
    assert "k_ends_count<true>" in kernel and "k_ends_count<false>" in kernel
    with open(os.path.join(CSRC, "ends.h")) as fh:
        includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", fh.read())
    assert includes == ['"liftmap.h"']                                                       # no GPU dependency
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    assert " ends.h " in make and " k_ends.hip " in make
    # the ends calls are not readers of the contact matrix, of a map build or of a span build
    ends_code = api[api.index("static void ends_abandon"):api.index("// Group support (DESIGN.md 9f)")]
    assert "hicmi_ends_file(" in ends_code
    for word in ("c->dC", "map_cells", "drop_matrix_state", "span_marks", "span_grid", "map_m"):
        assert word not in ends_code, word


# ---- the command line on a fake context ----------------------------------------------------------------------------------------------
class FakeContext:
    """``ends_file`` of _lib, answered by the reference on the file's pairs."""

    def __init__(self):
        self.calls = []

    def ends_file(self, path, names, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window, reach, threads=0):
        with open(path, "rb") as fh:
            pairs, stats, _after = bref.parse_text(fh.read(), names, sizes)
        tables = (np.asarray(lift_seq, np.int32), np.asarray(lift_off, np.int64), np.asarray(lift_rev, np.uint8), np.asarray(seq_sizes, np.int64))
        T, counters = ref.table(pairs, sizes, tables, window, reach)
        self.calls.append((int(window), int(reach)))
        return stats + (1,), ref.number_ranks(sizes, tables)[0], T, counters


@functools.lru_cache(maxsize=None)
def _planted():
    P = ref.planted()
    tables = lref.layout(P["chroms"], P["sizes"], 100, drop_unplaced=True)
    T, counters = ref.table(P["pairs"], P["sizes"], tables, ref.PLANTED_WINDOW, ref.PLANTED_REACH)
    T.setflags(write=False)
    return P, tables, T, counters


def test_planted_flips_on_the_reference_alone():
    """40 scaffolds of 6 to 64 kb in three chromosomes, ten of them - 6.2 kb ones, a chromosome's first and its last among
    them - given with the wrong sign: every one of them is called flip, every other scaffold supported.  The smallest
    |as_lies - flipped| over the 40 scaffolds is 30 (scaffold 40, 25 kb, the last of its chromosome: 6 against 36)."""
    P, tables, T, counters = _planted()
    rank, seq_first, n = ref.number_ranks(P["sizes"], tables)
    assert n == 40 and sorted(rank.tolist()) == list(range(40))
    verdicts, margin = {}, None
    for s in range(40):
        as_lies, flipped, alone = ref.scaffold_figures(T, seq_first, int(rank[s]))
        verdicts[s] = ref.scaffold_verdict(as_lies, flipped, alone, ref.PLANTED_MIN_PAIRS)
        margin = abs(as_lies - flipped) if margin is None else min(margin, abs(as_lies - flipped))
    assert len(P["flips"]) == 10 and min(P["sizes"][P["flips"]]) < 2 * ref.PLANTED_WINDOW < max(P["sizes"][P["flips"]])
    assert verdicts == {s: "flip" if s in P["flips"] else "supported" for s in range(40)}
    assert margin >= 20, margin
    # with the true signs nothing is to flip
    true_tables = lref.layout(P["true_chroms"], P["sizes"], 100, drop_unplaced=True)
    T0, _c = ref.table(P["pairs"], P["sizes"], true_tables, ref.PLANTED_WINDOW, ref.PLANTED_REACH)
    assert all(ref.scaffold_verdict(*ref.scaffold_figures(T0, seq_first, i), ref.PLANTED_MIN_PAIRS) == "supported" for i in range(40))
    assert all(ref.junction_verdict(ref.junction_figures(T0, i), ref.PLANTED_MIN_PAIRS) == "held"
               for q in range(3) for i in range(int(seq_first[q]), int(seq_first[q + 1]) - 1))


def _planted_files(tmp_path):
    from hic_genome_assembler_amd import synth
    P = _planted()[0]
    d = str(tmp_path)
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    with open(paths["hicProScaffSizeFile"], "w") as fh:
        fh.write("".join("%s\t%d\n" % ns for ns in zip(P["names"], P["sizes"].tolist())))
    pair_file = os.path.join(d, "planted.allValidPairs")
    with open(pair_file, "wb") as fh:
        fh.write(ref.pair_file_bytes(P["names"], P["pairs"]))
    order = os.path.join(d, "orders.txt")
    with open(order, "w") as fh:
        fh.write(lref.order_file_text(P["chroms"], P["names"]))
    save = os.path.join(d, "save")
    cfg = synth.write_config(os.path.join(d, "config.txt"), paths, save, os.path.join(d, "plots"), 100000, extra={"validPairFile": pair_file})
    return cfg, order, save, paths


def expected_report(names, sizes, chroms, pairs, window, reach, min_pairs, n_lines=None):
    """(report text, the scaffolds called flip, ends.links.tsv) from the reference."""
    tables = lref.layout(chroms, sizes, 100, drop_unplaced=True)
    T, counters = ref.table(pairs, sizes, tables, window, reach)
    rank, seq_first, _n = ref.number_ranks(sizes, tables)
    n_pairs = len(pairs[0])
    n_lines = n_pairs if n_lines is None else n_lines
    out = ["#window=%d\treach=%d\tminPairs=%d\tlines=%d\tused=%d\tunknown_scaffold=0\tout_of_range=0\t" % (window, reach, min_pairs, n_lines, n_pairs)
           + "\t".join("%s=%d" % kv for kv in zip(ref.COUNTERS, counters.tolist())),
           "#scaffold\torientation\tsize\tleft_zone\tright_zone\tas_lies\tflipped\tverdict"]
    flips, junctions, links = [], [], ["#scaffold\td\tneighbour\tleft_left\tleft_right\tright_left\tright_right"]
    for i, chrom in enumerate(chroms, 1):
        out.append("### Chromosome grouping %d ###" % i)
        filled = [s for s, _o in chrom if sizes[s] > 0]
        for s, o in chrom:
            if sizes[s] == 0:
                out.append("%s\t%s\t0\t0\t0\t0\t0\tNA" % (names[s], o))
                continue
            as_lies, flipped, alone = ref.scaffold_figures(T, seq_first, int(rank[s]))
            verdict = ref.scaffold_verdict(as_lies, flipped, alone, min_pairs)
            flips += [names[s]] if verdict == "flip" else []
            out.append("%s\t%s\t%d\t%d\t%d\t%d\t%d\t%s" % ((names[s], o, sizes[s]) + ref.zone_sizes(sizes[s], window) + (as_lies, flipped, verdict)))
        for k, (a, b) in enumerate(zip(filled, filled[1:])):
            figures = ref.junction_figures(T, int(rank[a]))
            junctions.append("%d\t%s\t%s\t%d\t%d\t%d\t%d\t%s" % ((i, names[a], names[b]) + figures + (ref.junction_verdict(figures, min_pairs),)))
        for k, a in enumerate(filled):
            for d in range(1, reach + 1):
                if k + d < len(filled):
                    links.append("%s\t%d\t%s\t%d\t%d\t%d\t%d" % ((names[a], d, names[filled[k + d]]) + tuple(T[rank[a], d - 1].tolist())))
    out += ["### Junctions ###", "#chromosome\tleft\tright\tfacing\tleft_flipped\tright_flipped\tboth_flipped\tverdict"] + junctions
    return "\n".join(out) + "\n", flips, "\n".join(links) + "\n"


def check_planted_outputs(report, flipped_text, links_text):
    """The outputs of the planted case against the reference (also used by the GPU round trip)."""
    P = _planted()[0]
    want, flips, links = expected_report(P["names"], P["sizes"], P["chroms"], P["pairs"], ref.PLANTED_WINDOW, ref.PLANTED_REACH,
                                         ref.PLANTED_MIN_PAIRS)
    assert report == want and links_text == links
    assert flips == [P["names"][s] for s in P["flips"]]
    # the flipped order file is the true one: every planted flip is undone, every other line is as it was
    assert flipped_text == lref.order_file_text(P["true_chroms"], P["names"])
    assert report.count("\tflip\n") == 10 and report.count("\tsupported\n") == 30 and "\topen\n" not in report


def _read(path):
    with open(path, newline="") as fh:
        return fh.read()


def test_cli_report_on_a_fake_context(tmp_path, capsys):
    from hic_genome_assembler_amd import supportEnds
    cfg, order, save, _paths = _planted_files(tmp_path)
    fake = FakeContext()
    flipped, full = str(tmp_path / "flipped.txt"), str(tmp_path / "full")
    supportEnds.main(["-config", cfg, "-order", order, "-window", "5000", "-flipped", flipped, "-full", full, "-threads", "2"], context=fake)
    assert fake.calls == [(5000, 2)]
    check_planted_outputs(_read(os.path.join(save, "endSupport.txt")), _read(flipped), _read(os.path.join(full, "ends.links.tsv")))
    assert "ENDS: 10 scaffold(s) to flip, 0 open" in capsys.readouterr().out


def test_cli_keeps_every_other_byte_of_the_order_file_and_reports_small_cases(tmp_path):
    """The six-scaffold assembly with an empty scaffold, an unplaced one, a chromosome of one scaffold, CR LF lines, a third
    column and no final newline."""
    from hic_genome_assembler_amd import supportEnds, synth
    d = str(tmp_path)
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    with open(paths["hicProScaffSizeFile"], "w") as fh:
        fh.write("".join("%s\t%d\n" % ns for ns in zip(NAMES, SIZES.tolist())))
    # c's far end (base 7, which lies first) is linked to b three times and to a's first base twice, its near end once: c
    # is the wrong way round.  b's one base is its left end: against one link through c's near end stand the two with a's
    # first base, which a turned b would have - flip.  a's own links all count for a neighbour: open.
    rows = [(C, 7, B, 1)] * 3 + [(A, 1, C, 7)] * 2 + [(C, 1, B, 1)] + [(A, 5, B, 1)] * 2 + [(A, 1, B, 1)] * 2 + [(E, 1, A, 1), (D, 1, A, 1), (C, 4, A, 1), (C, 2, C, 3)]
    pairs = _pairs(rows)
    pair_file = os.path.join(d, "small.allValidPairs")
    with open(pair_file, "wb") as fh:
        fh.write(ref.pair_file_bytes(NAMES, pairs))
    order = os.path.join(d, "orders.txt")
    text = "### Chromosome grouping 1 ###\r\nc\t-\tnote\r\nb\t-\r\na\t+\n### Chromosome grouping 2 ###\nd\t+\nf\t+"
    with open(order, "w", newline="") as fh:
        fh.write(text)
    save = os.path.join(d, "save")
    cfg = synth.write_config(os.path.join(d, "config.txt"), paths, save, os.path.join(d, "plots"), 100000, extra={"validPairFile": pair_file})
    out, flipped = os.path.join(d, "r.txt"), os.path.join(d, "flipped.txt")
    supportEnds.main(["-config", cfg, "-order", order, "-window", "1", "-reach", "2", "-minPairs", "2", "-out", out, "-flipped", flipped],
                     context=FakeContext())
    want, flips, _links = expected_report(NAMES, SIZES, CHROMS, pairs, 1, 2, 2)
    assert _read(out) == want and flips == ["c", "b"]
    lines = want.splitlines()
    assert lines[0].endswith("linked=10\tmiddle=1\tsame=1\ttoo_far=0\ttrans=1\tunlifted=1")
    assert lines[3:6] == ["c\t-\t7\t1\t1\t1\t5\tflip", "b\t-\t1\t1\t0\t1\t2\tflip", "a\t+\t5\t1\t1\t0\t0\topen"]
    assert lines[7:9] == ["d\t+\t3\t1\t1\t0\t0\tNA", "f\t+\t0\t0\t0\t0\t0\tNA"]
    assert lines[-2:] == ["1\tc\tb\t1\t3\t0\t0\tflip_left", "1\tb\ta\t0\t2\t0\t2\topen"]
    assert _read(flipped) == text.replace("c\t-\tnote", "c\t+\tnote").replace("b\t-\r", "b\t+\r")


def test_bad_input_is_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import supportEnds, synth
    cfg, order, save, paths = _planted_files(tmp_path)
    d = str(tmp_path)
    out = os.path.join(d, "report.txt")
    fake = FakeContext()

    def write(text, name):
        path = os.path.join(d, name)
        with open(path, "w") as fh:
            fh.write(text)
        return path

    def refused(word, more=(), config=cfg, order_file=order):
        args = ["-config", config, "-out", out, "-flipped", out + ".flipped", "-full", out + ".full"] + (["-order", order_file] if order_file else [])
        with pytest.raises(SystemExit) as exc:
            supportEnds.main(args + list(more), context=fake)
        assert word in str(exc.value.code) and str(exc.value.code).startswith("ERROR... ") and \
            str(exc.value.code).endswith(" Exiting..."), exc.value.code

    refused("window", ["-window", "0"])
    refused("window", ["-window", "-5"])
    refused("reach", ["-reach", "0"])
    refused("reach", ["-reach", "65"])
    refused("minPairs", ["-minPairs", "-1"])
    refused("zz", order_file=write("### 1 ###\nscaf_1\t+\nzz\t+\n", "unknown.txt"))
    refused("twice", order_file=write("### 1 ###\nscaf_1\t+\n### 2 ###\nscaf_2\t+\nscaf_1\t-\n", "twice.txt"))
    refused("orientation", order_file=write("### 1 ###\nscaf_1\t+\nscaf_2\t?\n", "orient.txt"))
    refused("no scaffold", order_file=write("### 1 ###\nscaf_1\t+\n### 2 ###\n", "empty.txt"))
    refused("orientation column", order_file=write("### 1 ###\nscaf_1\n", "one_column.txt"))
    refused("does not exist", order_file=os.path.join(d, "nothing_here"))
    refused("does not exist", order_file=None)                               # neither default order file is there
    # 2^19 + 1 placed scaffolds at reach 64: one entry past the table
    n = 2 ** 19 + 1
    big = dict(paths, hicProScaffSizeFile=write("".join("s%d\t1\n" % k for k in range(n)), "big.sizes"))
    big_cfg = synth.write_config(os.path.join(d, "big.txt"), big, save, os.path.join(d, "plots"), 100000,
                                 extra={"validPairFile": os.path.join(d, "planted.allValidPairs")})
    big_order = write("### 1 ###\n" + "".join("s%d\t+\n" % k for k in range(n)), "big.order")
    refused("%d counters" % (n * 256), ["-reach", "64"], config=big_cfg, order_file=big_order)
    refused("validPairFile", config=synth.write_config(os.path.join(d, "c2.txt"), paths, save, os.path.join(d, "plots"), 100000))
    missing = synth.write_config(os.path.join(d, "c3.txt"), paths, save, os.path.join(d, "plots"), 100000,
                                 extra={"validPairFile": os.path.join(d, "no_such_pairs")})
    refused("validPairFile", config=missing)
    assert fake.calls == [] and os.listdir(save) == []
    assert not any(os.path.exists(p) for p in (out, out + ".flipped", out + ".full"))
