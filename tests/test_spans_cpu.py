"""supportSpans without a GPU: tests/span_reference.py against its own brute-force depth and hand-worked
cases, csrc/span.h built as host code with the sanitizers and compared line by line with the reference, the declarations,
the report and the refusals of the command line on a fake context that answers from the reference, and the planted
misjoin.  Every comparison is exact."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import liftmap_reference as lref
import span_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")

# six scaffolds a .. f; Chr_1 = c-, b-, a+ (b has one base), Chr_2 = d+, f+ (f has no base), e is not placed
NAMES = ["a", "b", "c", "d", "e", "f"]
SIZES = np.array([5, 1, 7, 3, 4, 0], dtype=np.int64)
CHROMS = [[(2, "-"), (1, "-"), (0, "+")], [(3, "+"), (5, "+")]]


# ---- the reference against itself and hand-worked cases ----------------------------------------------------------------------
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", [0, 1, 100])
def test_cell_numbering_against_hand_worked_cases(gap, drop):
    tables = lref.layout(CHROMS, SIZES, gap, drop_unplaced=drop)
    # step 2: c has 4 cells (the last one, its base 1, of 1 bp), b is one cell, a has 3 (the last of 1 bp); d has 2, f none
    cell_first, seq_first, n = ref.number_cells(SIZES, tables, 2)
    assert cell_first.tolist() == [5, 4, 0, 8, -1 if drop else 10, -1] and n == (10 if drop else 12)
    assert seq_first.tolist() == ([0, 8, 10] if drop else [0, 8, 10, 12])
    ends = [(s, p) for s in (0, 1, 2, 3) for p in range(1, int(SIZES[s]) + 1)]
    pairs = tuple(np.array(x) for x in zip(*[(s, p, s, p) for s, p in ends]))
    ca, _cb = ref.cells(pairs, SIZES, tables, cell_first, 2)
    #                    a: bases 1 .. 5      b    c (reversed): bases 1 .. 7      d: 1 .. 3
    assert ca.tolist() == [5, 5, 6, 6, 7] + [4] + [3, 2, 2, 1, 1, 0, 0] + [8, 8, 9]
    # a step as long as the longest scaffold, and a longer one: one cell each
    for step in (7, 1000):
        cell_first, seq_first, n = ref.number_cells(SIZES, tables, step)
        assert cell_first.tolist() == [2, 1, 0, 3, -1 if drop else 4, -1] and n == (4 if drop else 5)
    # step 1: a cell per base
    assert ref.number_cells(SIZES, tables, 1)[0].tolist() == [8, 7, 0, 13, -1 if drop else 16, -1]


@pytest.mark.parametrize("gap", [0, 1, 100])
def test_a_pair_across_a_junction_counts_at_the_junction_slot_only(gap):
    tables = lref.layout(CHROMS, SIZES, gap)
    # base 1 of c is the last base of c as it lies in Chr_1, base 1 of b the first one of b: the pair spans the junction
    pairs = (np.array([2]), np.array([1]), np.array([1]), np.array([1]))
    D, counters, marks = ref.depth(pairs, SIZES, tables, 2)
    assert D.tolist() == [0, 0, 0, 1] + [0] * 8 and counters.tolist() == [1, 0, 0, 0, 0]      # 12 cells whatever the gap is
    assert marks[3] == 1 and marks[4] == np.uint64(2 ** 64 - 1)
    scaf, junc = ref.report_records(SIZES, tables, 2)
    assert junc == {(2, 1): (3, 3, 0, 8), (1, 0): (4, 4, 0, 8)} and scaf == {2: (0, 2, 0, 8), 0: (5, 6, 0, 8), 3: (8, 8, 8, 10), 4: (10, 10, 10, 12)}
    # from the far end of c to the far end of a: every slot of Chr_1 but its terminator
    D, _counters, _marks = ref.depth((np.array([2]), np.array([7]), np.array([0]), np.array([5])), SIZES, tables, 2)
    assert D.tolist() == [1] * 7 + [0] * 5
    # the distance limit is measured in the assembly: 1 + gap between the two bases of the junction
    for max_span, counted in ((gap + 1, 1), (gap, 0) if gap else (5, 1)):
        D, counters, _marks = ref.depth(pairs, SIZES, tables, 2, max_span)
        assert int(D[3]) == counted and counters.tolist() == [counted, 0, 1 - counted, 0, 0]


def _random_case(seed):
    rng = np.random.default_rng(seed)
    S = int(rng.integers(3, 12))
    sizes = rng.integers(0, 30, S).astype(np.int64)
    order = rng.permutation(S).tolist()
    n_placed = int(rng.integers(2, S + 1))
    cut = int(rng.integers(1, n_placed))
    chroms = [[(s, "+-"[int(rng.integers(0, 2))]) for s in part] for part in (order[:cut], order[cut:n_placed])]
    tables = lref.layout(chroms, sizes, int(rng.choice([0, 1, 100])), drop_unplaced=bool(rng.integers(0, 2)))
    have = np.flatnonzero(sizes > 0)
    n = 300
    sa, sb = rng.choice(have, n), rng.choice(have, n)
    near = rng.random(n) < 0.5
    sb[near] = sa[near]
    pa = 1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64)
    return sizes, tables, (sa.astype(np.int32), pa, sb.astype(np.int32), pb), int(rng.choice([1, 3, 7])), int(rng.choice([0, 0, 5, 40]))


@pytest.mark.parametrize("seed", range(12))
def test_reference_depth_equals_the_brute_force_depth(seed):
    sizes, tables, pairs, step, max_span = _random_case(seed)
    D, counters, marks = ref.depth(pairs, sizes, tables, step, max_span)
    assert D.dtype == np.uint64 and D.tobytes() == ref.brute_depth(pairs, sizes, tables, step, max_span).tobytes()
    assert int(counters.sum()) == len(pairs[0]) and int(marks.sum(dtype=np.uint64)) == 0
    _cell_first, seq_first, n = ref.number_cells(sizes, tables, step)
    assert len(D) == n and not D[seq_first[1:][seq_first[1:] > seq_first[:-1]] - 1].any()           # 0 at every terminator


def test_the_random_cases_hold_every_kind_of_pair():
    total = np.zeros(5, np.uint64)
    for seed in range(12):
        sizes, tables, pairs, step, max_span = _random_case(seed)
        total += ref.depth(pairs, sizes, tables, step, max_span)[1]
    assert (total > 20).all(), total


def test_ratio_division_and_first_minimum():
    D = np.array([5, 5, 5, 2, 5, 5, 1, 5, 5, 5, 0], np.uint64)
    comp, ls, rs = ref.flanks(D, 2, 0, 11)
    assert np.flatnonzero(comp).tolist() == [2, 3, 4, 5, 6, 7]                       # c - 2 >= 0 and c + 2 <= 9
    assert (ls[3], rs[3], ls[4], rs[4], ls[6], rs[6]) == (10, 10, 7, 6, 10, 10)
    got = ref.picks(D, 2, [(0, 10, 0, 11), (0, 5, 0, 11), (4, 4, 0, 11), (0, 1, 0, 11), (8, 10, 0, 11)])
    assert got.tolist() == [[6, 1, 10, 10], [3, 2, 10, 10], [4, 5, 7, 6], [-1, 0, 0, 0], [-1, 0, 0, 0]]
    assert ref.pick_ratio(got[0], 2) == 2 / 10 and ref.pick_ratio(got[1], 2) == 4 / 10 and ref.pick_ratio(got[2], 2) == 10 / 6
    assert ref.pick_ratio(got[3], 2) is None
    # equal ratios: the first slot wins
    D = np.array([4, 4, 1, 4, 4, 1, 4, 4, 0], np.uint64)
    assert ref.picks(D, 2, [(0, 8, 0, 9), (3, 8, 0, 9)]).tolist() == [[2, 1, 8, 8], [5, 1, 8, 8]]
    # inside a longer array, the flanks stop at the sequence: [3, 12) here
    D = np.concatenate([[9, 9, 0], D]).astype(np.uint64)
    assert ref.picks(D, 2, [(3, 11, 3, 12)]).tolist() == [[5, 1, 8, 8]]
    # a flank that sums to zero does not compete
    D = np.array([0, 0, 3, 3, 3, 0], np.uint64)
    assert ref.picks(D, 2, [(0, 5, 0, 6)]).tolist() == [[-1, 0, 0, 0]]
    # the division is the IEEE one of the two integers
    assert ref.ratio(3, 7, 2 ** 40 + 1, 2 ** 41) == 21 / (2 ** 40 + 1) and ref.ratio(2 ** 49, 8, 2 ** 52 + 1, 2 ** 53 - 1) == float(2 ** 52) / float(2 ** 52 + 1)


# ---- span.h as host code under the sanitizers -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("spans") / "span_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "span_host_check.cpp"), "-o", exe])

    def run(path, sizes, tables, step, max_span, flank, pairs, recs):
        seq, off, rev, seq_sizes = tables
        lines = ["T %d %d %d %d %d" % (len(sizes), len(seq_sizes), step, max_span, flank)]
        lines += ["%d %d %d %d" % row for row in zip(map(int, sizes), map(int, seq), map(int, off), map(int, rev))]
        lines += [" ".join(str(int(x)) for x in seq_sizes), "P %d" % len(pairs[0])]
        lines += ["%d %d %d %d" % row for row in zip(*(np.asarray(x).tolist() for x in pairs))]
        lines += ["R %d" % len(recs)] + ["%d %d %d %d" % tuple(r) for r in recs]
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        # an ordinary child process, nothing preloaded
        done = subprocess.run([exe, path], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        return done.stdout.splitlines()
    return run


def _expected_lines(sizes, tables, step, max_span, flank, pairs, recs):
    cell_first, seq_first, n = ref.number_cells(sizes, tables, step)
    kind, lo, hi = ref.classify(pairs, sizes, tables, cell_first, step, max_span)
    D, _counters, _marks = ref.depth(pairs, sizes, tables, step, max_span)
    out = ["check 0 ", "cells %d" % n] + ["first %d" % c for c in cell_first] + ["seq %d" % c for c in seq_first]
    out += ["pair %d %d %d" % (k, a if k == 0 else -1, b if k == 0 else -1) for k, a, b in zip(kind.tolist(), lo.tolist(), hi.tolist())]
    out += ["depth %d" % d for d in D.tolist()]
    return out, ref.picks(D, flank, recs)


def _same_as_the_reference(got, sizes, tables, step, max_span, flank, pairs, recs):
    want, picks = _expected_lines(sizes, tables, step, max_span, flank, pairs, recs)
    assert got[:len(want)] == want and len(got) == len(want) + len(recs)
    for line, pick in zip(got[len(want):], picks.tolist()):
        cols = line.split()
        assert cols[0] == "pick" and [int(x) for x in cols[1:5]] == pick
        assert (cols[5] == "NA") if pick[0] < 0 else (float.fromhex(cols[5]) == ref.pick_ratio(pick, flank))


@pytest.mark.parametrize("seed", range(12))
def test_native_cells_marks_and_picks_under_the_sanitizers(seed, host_check, tmp_path):
    sizes, tables, pairs, step, max_span = _random_case(seed)
    _cell_first, seq_first, n = ref.number_cells(sizes, tables, step)
    rng = np.random.default_rng(seed + 100)
    recs = []
    for q in range(len(seq_first) - 1):
        q0, q1 = int(seq_first[q]), int(seq_first[q + 1])
        if q1 > q0:
            recs.append((q0, q1 - 1, q0, q1))
            lo = int(rng.integers(q0, q1))
            recs.append((lo, int(rng.integers(lo, q1)), q0, q1))
    for flank in (1, 2, 5):
        got = host_check(str(tmp_path / "case.txt"), sizes, tables, step, max_span, flank, pairs, recs)
        _same_as_the_reference(got, sizes, tables, step, max_span, flank, pairs, recs)


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", [0, 1, 100])
def test_native_hand_worked_numbering_under_the_sanitizers(gap, drop, host_check, tmp_path):
    tables = lref.layout(CHROMS, SIZES, gap, drop_unplaced=drop)
    ends = [(s, p) for s in range(5) for p in range(1, int(SIZES[s]) + 1)]
    pairs = tuple(np.array(x) for x in zip(*[a + b for a in ends for b in ends]))           # every end against every end
    for step in (1, 2, 3, 7, 1000):
        for max_span in (0, 3):
            got = host_check(str(tmp_path / "case.txt"), SIZES, tables, step, max_span, 1, pairs, [(0, 0, 0, int(ref.number_cells(SIZES, tables, step)[1][1]))])
            _same_as_the_reference(got, SIZES, tables, step, max_span, 1, pairs, [(0, 0, 0, int(ref.number_cells(SIZES, tables, step)[1][1]))])
    assert got[1] == ("cells 4" if drop else "cells 5")


def test_native_positions_above_2_to_the_32_under_the_sanitizers(host_check, tmp_path):
    L = 2 ** 33
    sizes = np.array([L, L, L, 5], dtype=np.int64)
    tables = lref.layout([[(0, "+"), (1, "-"), (2, "+")]], sizes, 100)
    step = 2 ** 20
    edge = [1, 2, step, step + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, L - step, L - step + 1, L - 1, L]
    ends = [(s, p) for s in range(3) for p in edge] + [(3, 1), (3, 5)]
    pairs = tuple(np.array(x) for x in zip(*[a + b for a in ends for b in ends]))
    cell_first, seq_first, n = ref.number_cells(sizes, tables, step)
    assert n == 3 * 8192 + 1 and cell_first.tolist() == [0, 8192, 16384, 24576]
    recs = [(0, n - 2, 0, n - 1), (8191, 8191, 0, n - 1), (8192, 16382, 0, n - 1), (24576, 24576, 24576, 24577)]
    for max_span, flank in ((0, 8), (2 ** 32, 4096), (2 ** 33 + 100, 1)):
        got = host_check(str(tmp_path / "case.txt"), sizes, tables, step, max_span, flank, pairs, recs)
        _same_as_the_reference(got, sizes, tables, step, max_span, flank, pairs, recs)
    # more than 2^27 cells: refused by the numbering, and nothing after it is printed
    got = host_check(str(tmp_path / "case.txt"), sizes, tables, 64, 0, 1, pairs, [])
    assert got == ["check 0 ", "cells -1"]
    # 3 ceil(2^33 / 192) + 1 = 2^27 + 2 cells: just past the limit
    assert 3 * (-(-L // 192)) + 1 == 2 ** 27 + 2
    assert host_check(str(tmp_path / "case.txt"), sizes, tables, 192, 0, 1, pairs, []) == ["check 0 ", "cells -1"]


# ---- header, binding, switch ---------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_exports():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = re.sub(r"\s+", " ", fh.read())
    tables = "const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq"
    assert ("int hicmi_span_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, " + tables + ", int64_t step, "
            "int64_t max_span, int64_t *cell_first_out, int64_t *n_cells_out);") in text
    assert ("int hicmi_span_add_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b, "
            "const int64_t *pos_b, int64_t n);") in text
    assert ("int hicmi_span_finish(hicmi_ctx *ctx, int64_t flank, const int64_t *recs, int64_t n_rec, int64_t *picks_out, "
            "uint64_t *counters5_out, uint64_t *depth_out);") in text
    assert ("int hicmi_span_file(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names, "
            "const int64_t *scaf_size, " + tables + ", int64_t step, int64_t max_span, int64_t flank, const int64_t *recs, "
            "int64_t n_rec, hicmi_ctx *ctx, int threads, int64_t *stats5, int64_t *picks_out, uint64_t *counters5_out, "
            "uint64_t *depth_out, int64_t *cell_first_out, int64_t *n_cells_out);") in text
    lib = _lib.load()
    for name, n_args in {"hicmi_span_begin": 12, "hicmi_span_add_pairs": 6, "hicmi_span_finish": 7, "hicmi_span_file": 23}.items():
        assert len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
    for method in ("span_begin", "span_add_pairs", "span_finish"):
        assert callable(getattr(_lib.Context, method))
    assert callable(_lib.span_file) and lib.hicmi_abi_version() == 1
    assert set(_lib.SIGNATURES) == set(re.findall(r"\b(hicmi_[a-z0-9_]+)\(", text)) - {"hicmi_ctx"}


def test_the_mark_form_is_read_at_every_call_and_the_constants_are_named():
    with open(os.path.join(CSRC, "api.hip")) as fh:
        api = fh.read()
    assert 'getenv("HICMI_SPANS_PLAIN")' in api and api.count("spans_plain()") == 3        # a definition and two uses
    for path in (os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))):
        with open(path) as fh:
            assert not [ln for ln in fh if "HICMI_SPANS_PLAIN" in ln and re.search(r"\bstatic\b[^;]*\bgetenv\(", ln)], path
    with open(os.path.join(CSRC, "hicmi_internal.h")) as fh:
        internal = fh.read()
    for name in ("SPAN_SCAN_TILE", "SPAN_SCAN_WIDTH", "SPAN_SLICE", "SPAN_SLOTS"):
        assert re.search(r"static constexpr int %s = " % name, internal), name
    with open(os.path.join(CSRC, "span.h")) as fh:
        includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", fh.read())
    assert includes == ['"liftmap.h"']                                                       # no GPU dependency
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    assert " span.h " in make and " k_spans.hip " in make
    # the span calls are not readers of the contact matrix
    span_code = api[api.index("static void span_abandon"):api.index("// Group support (DESIGN.md 9f)")]
    assert "c->dC" not in span_code and "map_cells" not in span_code and "drop_matrix_state" not in span_code


# ---- the command line on a fake context ----------------------------------------------------------------------------------------------
class FakeContext:
    """The span calls of _lib.Context, answered by the reference."""

    def __init__(self):
        self.build, self.calls = None, []

    def span_begin(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, step, max_span=0):
        tables = (np.asarray(lift_seq, np.int32), np.asarray(lift_off, np.int64), np.asarray(lift_rev, np.uint8), np.asarray(seq_sizes, np.int64))
        self.build = [np.asarray(sizes, np.int64), tables, int(step), int(max_span), [[], [], [], []]]
        self.calls.append("begin")
        return ref.number_cells(sizes, tables, step)[0]

    def span_add_pairs(self, sa, pa, sb, pb):
        for have, more in zip(self.build[4], (sa, pa, sb, pb)):
            have.append(np.asarray(more))
        self.calls.append("add")

    def span_finish(self, flank, recs, want_depth=True):
        sizes, tables, step, max_span, parts = self.build
        pairs = tuple(np.concatenate(p) for p in parts)
        D, counters, _marks = ref.depth(pairs, sizes, tables, step, max_span)
        self.build = None
        self.calls.append("finish")
        return ref.picks(D, flank, recs), counters, D if want_depth else None


@functools.lru_cache(maxsize=None)
def _planted():
    P = ref.planted()
    tables = lref.layout(P["chroms"], P["sizes"], 100)
    D, counters, _marks = ref.depth(P["pairs"], P["sizes"], tables, ref.PLANTED_STEP)
    scaf, junc = ref.report_records(P["sizes"], tables, ref.PLANTED_STEP)
    keys = list(scaf) + list(junc)
    picks = ref.picks(D, ref.PLANTED_FLANK, [scaf[k] for k in scaf] + [junc[k] for k in junc])
    D.setflags(write=False)
    return P, tables, D, counters, dict(zip(keys, picks.tolist()))


def test_planted_misjoin_on_the_reference_alone():
    """The glued joint and the false junction have a ratio below minRatio; every other scaffold and junction that competes
    has one at or above it."""
    P, tables, D, counters, picks = _planted()
    glued, false_junction = P["glued"], P["false_junction"]
    cell_first, _seq_first, _n = ref.number_cells(P["sizes"], tables, ref.PLANTED_STEP)
    assert picks[glued][0] == cell_first[glued] + P["glue_at"] // ref.PLANTED_STEP - 1
    low = {k for k, p in picks.items() if p[0] >= 0 and ref.pick_ratio(p, ref.PLANTED_FLANK) < ref.PLANTED_MIN_RATIO}
    assert low == {glued, false_junction}
    competing = [k for k, p in picks.items() if p[0] >= 0]
    assert len(competing) >= len(picks) - 1 and picks[P["contig"]][0] == -1               # the 12-cell contig has no room for the flanks
    assert all(ref.pick_ratio(picks[k], ref.PLANTED_FLANK) >= 2 * ref.PLANTED_MIN_RATIO for k in competing if k not in low)
    assert counters[0] > 30000 and counters[3] > 300 and counters[4] == 0


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


def check_planted_report(text, cuts_text, full_text, scaffolds_only=False):
    """The report of the planted case against the reference (also used by the GPU round trip)."""
    P, tables, D, counters, picks = _planted()
    names, sizes, F = P["names"], P["sizes"], ref.PLANTED_FLANK
    n_pairs = len(P["pairs"][0])
    lines = text.splitlines()
    assert lines[0] == "#step=1000\tmaxSpan=0\tflank=8\tminRatio=0.2\tlines=%d\tused=%d\tunknown_scaffold=0\tout_of_range=0\t" % (n_pairs, n_pairs) \
        + "\t".join("%s=%d" % kv for kv in zip(ref.COUNTERS, counters.tolist()))
    assert lines[1] == "#scaffold\torientation\tsize\tcells\tcut_after\tdepth\tflank_depth\tratio\tverdict"

    def scaffold_cols(s, o):
        L, p = int(sizes[s]), picks.get(s)
        head = [names[s], o, str(L), str(-(-L // 1000))]
        if p is None or p[0] < 0:
            return head + ["NA"] * 5
        cell_first = ref.number_cells(sizes, tables, 1000)[0]
        inside = (p[0] - int(cell_first[s]) + 1) * 1000
        r = ref.pick_ratio(p, F)
        return head + [str(L - inside if o == "-" else inside), str(p[1]), repr(min(p[2], p[3]) / F), repr(r), "suspect" if r < 0.2 else "spanned"]

    want = []
    for i, chrom in enumerate(P["chroms"], 1):
        want.append("### Chromosome grouping %d ###" % i)
        want += ["\t".join(scaffold_cols(s, o)) for s, o in chrom]
    want += ["### Junctions ###", "#chromosome\tleft\tright\tdepth\tflank_depth\tratio\tverdict"]
    for i, chrom in enumerate(P["chroms"], 1):
        for (a, _oa), (b, _ob) in zip(chrom, chrom[1:]):
            p = picks[(a, b)]
            r = ref.pick_ratio(p, F)
            want.append("\t".join([str(i), names[a], names[b], str(p[1]), repr(min(p[2], p[3]) / F), repr(r), "weak" if r < 0.2 else "held"]))
    want += ["### Unplaced ###", "\t".join(scaffold_cols(P["contig"], "+"))]
    assert lines[2:] == want
    glued = scaffold_cols(P["glued"], "+")
    assert glued[4] == str(P["glue_at"]) and glued[8] == "suspect" and cuts_text == "%s\t%s\t%s\n" % (glued[0], glued[4], glued[7])
    assert sum(ln.endswith("\tweak") for ln in lines) == 1 and sum(ln.endswith("\tsuspect") for ln in lines) == 1
    assert sum(ln.endswith("\tNA") for ln in lines) == 1 and any("\t-\t" in ln for ln in lines[:20])
    # the depth of every cell, in the coordinates of the assembly
    full = [ln.split("\t") for ln in full_text.splitlines()]
    assert full[0] == ["#sequence", "first_base", "last_base", "depth"] and [int(r[3]) for r in full[1:]] == D.tolist()
    first = P["chroms"][0][0][0]
    assert full[1][:3] == ["Chr_1", "1", "1000"] and full[int(sizes[first]) // 1000 + 1][:3] == ["Chr_1", str(int(sizes[first]) + 101), str(int(sizes[first]) + 1100)]
    assert full[-1][:3] == [names[P["contig"]], "11001", "12000"]


def test_cli_report_on_a_fake_context(tmp_path, capsys):
    from hic_genome_assembler_amd import supportSpans
    cfg, order, save, _paths = _planted_files(tmp_path)
    fake = FakeContext()
    cuts, full = str(tmp_path / "cuts.tsv"), str(tmp_path / "full")
    supportSpans.main(["-config", cfg, "-order", order, "-step", "1000", "-cuts", cuts, "-full", full, "-threads", "2"], context=fake)
    assert fake.calls == ["begin", "add", "finish"] and fake.build is None
    with open(os.path.join(save, "spanSupport.txt")) as fh, open(cuts) as fc, open(os.path.join(full, "spans.depth.tsv")) as ff:
        check_planted_report(fh.read(), fc.read(), ff.read())
    assert "SPANS: 1 scaffold(s) suspect, 1 of 12 junction(s) weak" in capsys.readouterr().out


def test_cli_scaffolds_only_on_a_fake_context(tmp_path):
    from hic_genome_assembler_amd import supportSpans
    P = _planted()[0]
    cfg, _order, _save, _paths = _planted_files(tmp_path)
    out, cuts = str(tmp_path / "own.txt"), str(tmp_path / "cuts.tsv")
    supportSpans.main(["-config", cfg, "-scaffolds", "-step", "1000", "-flank", "5", "-out", out, "-cuts", cuts], context=FakeContext())
    tables = lref.identity(P["sizes"])
    D, _counters, _marks = ref.depth(P["pairs"], P["sizes"], tables, 1000)
    scaf, junc = ref.report_records(P["sizes"], tables, 1000)
    assert not junc
    with open(out) as fh:
        lines = fh.read().splitlines()
    assert lines[2] == "### Scaffolds ###" and len(lines) == 3 + len(P["names"]) and not any(ln.startswith("### J") for ln in lines)
    for s, line in enumerate(lines[3:]):
        cols = line.split("\t")
        p = ref.picks(D, 5, [scaf[s]])[0].tolist()
        assert cols[:4] == [P["names"][s], "+", str(int(P["sizes"][s])), str(-(-int(P["sizes"][s]) // 1000))]
        if p[0] < 0:
            assert cols[4:] == ["NA"] * 5
        else:
            r = ref.pick_ratio(p, 5)
            assert cols[4:] == [str((p[0] - scaf[s][2] + 1) * 1000), str(p[1]), repr(min(p[2], p[3]) / 5), repr(r), "suspect" if r < 0.2 else "spanned"]
    # on its own, the glued scaffold is cut at its joint
    glued = lines[3 + P["glued"]].split("\t")
    with open(cuts) as fh:
        assert glued[4] == str(P["glue_at"]) and glued[8] == "suspect" and fh.read() == "%s\t%s\t%s\n" % (glued[0], glued[4], glued[7])


def test_bad_input_is_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import supportSpans, synth
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
        args = ["-config", config, "-out", out, "-cuts", out + ".cuts", "-full", out + ".full"] + (["-order", order_file] if order_file else [])
        with pytest.raises(SystemExit) as exc:
            supportSpans.main(args + list(more), context=fake)
        assert word in str(exc.value.code) and str(exc.value.code).startswith("ERROR... ") and \
            str(exc.value.code).endswith(" Exiting..."), exc.value.code

    refused("step", ["-step", "0"])
    refused("step", ["-step", "-5"])
    refused("flank", ["-flank", "0"])
    refused("flank", ["-flank", "4097"])
    refused("maxSpan", ["-maxSpan", "-1"])
    refused("negative", ["-gap", "-1"])
    refused("no order file", ["-scaffolds"])
    refused("zz", order_file=write("### 1 ###\nscaf_1\t+\nzz\t+\n", "unknown.txt"))
    refused("twice", order_file=write("### 1 ###\nscaf_1\t+\n### 2 ###\nscaf_2\t+\nscaf_1\t-\n", "twice.txt"))
    refused("orientation", order_file=write("### 1 ###\nscaf_1\t+\nscaf_2\t?\n", "orient.txt"))
    refused("no scaffold", order_file=write("### 1 ###\nscaf_1\t+\n### 2 ###\n", "empty.txt"))
    refused("orientation column", order_file=write("### 1 ###\nscaf_1\n", "one_column.txt"))
    refused("does not exist", order_file=os.path.join(d, "nothing_here"))
    refused("does not exist", order_file=None)                               # neither default order file is there
    # 2^27 + 1 cells
    big = dict(paths, hicProScaffSizeFile=write("scaf_1\t%d\nscaf_2\t1\n" % 2 ** 27, "big.sizes"))
    big_cfg = synth.write_config(os.path.join(d, "big.txt"), big, save, os.path.join(d, "plots"), 100000,
                                 extra={"validPairFile": os.path.join(d, "planted.allValidPairs")})
    refused("%d cells" % (2 ** 27 + 1), ["-step", "1", "-scaffolds"], config=big_cfg, order_file=None)
    refused("validPairFile", config=synth.write_config(os.path.join(d, "c2.txt"), paths, save, os.path.join(d, "plots"), 100000))
    assert fake.calls == [] and os.listdir(save) == []
    assert not any(os.path.exists(p) for p in (out, out + ".cuts", out + ".full"))
