"""placeUnplaced without a GPU: tests/anchor_reference.py against its own brute-force table and hand-worked
cases, csrc/anchor.h built as host code with the sanitizers and compared line by line with the reference, the declarations,
and the command line - every verdict, the report, the ``-placed`` file and the refusals - on a NumPy stand-in context that
answers the array calls from the reference.  Every comparison is exact."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import anchor_reference as ref
import buildmap_reference as bref
import liftmap_reference as lref
from test_gpu_ends import CHROMS as ODD_CHROMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")


def _pairs(rows):
    sa, pa, sb, pb = zip(*rows)
    return (np.array(sa, np.int32), np.array(pa, np.int64), np.array(sb, np.int32), np.array(pb, np.int64))


# ---- the reference against itself and hand-worked cases ----------------------------------------------------------------------
# six scaffolds: Chr_1 = c-, a+ ; Chr_2 = d+ ; b (1 base), e (4 bases) and f (no base) are not placed
SIZES = np.array([5, 1, 7, 3, 4, 0], dtype=np.int64)
SMALL = [[(2, "-"), (0, "+")], [(3, "+")]]
A, B, C, D, E, F = range(6)


def test_blocks_against_hand_worked_cases():
    tables = lref.layout(SMALL, SIZES, 100, drop_unplaced=True)
    first, n = ref.number_blocks(SIZES, tables)
    assert first.tolist() == [-1, 0, -1, -1, 2, -1] and n == 4                   # b and e, two sequences each; f has no base
    first, n = ref.number_blocks(SIZES, tables, [-1, 1, -1, -1, 0, -1])
    assert first.tolist() == [-1, 0, -1, -1, 4, -1] and n == 4 * 1 + 4 * 2       # b against d alone, e against c and a
    first, n = ref.number_blocks(SIZES, tables, [-1, -1, -1, -1, 0, -1])
    assert first.tolist() == [-1, -1, -1, -1, 0, -1] and n == 8


def test_a_pair_lands_where_the_definitions_say():
    tables = lref.layout(SMALL, SIZES, 100, drop_unplaced=True)
    # sequence mode: e with a (Chr_1), e with d (Chr_2), b with c; either mate order
    for pairs in (_pairs([(E, 1, A, 2), (D, 3, E, 4), (B, 1, C, 7)]), _pairs([(A, 2, E, 1), (E, 4, D, 3), (C, 7, B, 1)])):
        T, counters = ref.table(pairs, SIZES, tables, None, 1)
        assert T.tolist() == [1, 0, 1, 1] and counters.tolist() == [3, 0, 0, 0, 0, 0]
    # rank mode, window 1: e (4 bases: 1, 2 first half, 3, 4 second half) against Chr_1 = c- (rank 0), a+ (rank 1)
    target = [-1, -1, -1, -1, 0, -1]
    rows = [(E, 2, C, 7),      # c is reversed: base 7 lies first, its LEFT zone -> k 0, zu 0, zp LEFT
            (E, 3, C, 1),      # base 1 of c lies last: RIGHT -> k 0, zu 1, zp RIGHT
            (A, 5, E, 4),      # a+: base 5 is its last: RIGHT -> k 1, zu 1, zp RIGHT
            (E, 1, A, 3),      # the middle of a
            (E, 1, D, 1),      # d lies in Chr_2: elsewhere
            (B, 1, A, 1),      # b has no target: skipped
            (B, 1, E, 1), (E, 1, E, 4),   # neither end lifts
            (A, 1, C, 1)]      # both lift
    T, counters = ref.table(_pairs(rows), SIZES, tables, target, 1)
    want = np.zeros(8, np.uint64)
    want[0 * 4 + 0 * 2 + ref.LEFT] = want[0 * 4 + 1 * 2 + ref.RIGHT] = want[1 * 4 + 1 * 2 + ref.RIGHT] = 1
    assert T.tobytes() == want.tobytes() and counters.tolist() == [3, 1, 1, 1, 2, 1]
    assert ref.halves([E] * 4 + [A] * 5 + [B], [1, 2, 3, 4, 1, 2, 3, 4, 5, 1], SIZES).tolist() == [0, 0, 1, 1, 0, 0, 0, 1, 1, 0]


def _random_case(seed):
    rng = np.random.default_rng(seed)
    S = int(rng.integers(5, 14))
    sizes = rng.integers(0, 30, S).astype(np.int64)
    order = rng.permutation(S).tolist()
    n_placed = int(rng.integers(2, S - 1))
    cut = int(rng.integers(1, n_placed))
    chroms = [[(s, "+-"[int(rng.integers(0, 2))]) for s in part] for part in (order[:cut], order[cut:n_placed])]
    tables = lref.layout(chroms, sizes, int(rng.choice([0, 1, 100])), drop_unplaced=True)
    rank_mode = bool(seed % 2)
    target = None
    if rank_mode:
        filled = [any(sizes[s] > 0 for s, _o in ch) for ch in chroms]
        target = np.full(S, -1, np.int32)
        for s in order[n_placed:]:
            q = int(rng.integers(-1, 2))
            if sizes[s] > 0 and q >= 0 and filled[q]:
                target[s] = q
        if not (target >= 0).any():
            return _random_case(seed + 1000)
    elif not any(sizes[s] > 0 for s in order[n_placed:]):
        return _random_case(seed + 1000)
    have = np.flatnonzero(sizes > 0)
    n = 400
    sa, sb = rng.choice(have, n), rng.choice(have, n)
    pa = 1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64)
    return sizes, tables, target, (sa.astype(np.int32), pa, sb.astype(np.int32), pb), int(rng.choice([1, 4, 9, 1000]))


@pytest.mark.parametrize("seed", range(12))
def test_reference_table_equals_the_brute_force_table(seed):
    sizes, tables, target, pairs, window = _random_case(seed)
    T, counters = ref.table(pairs, sizes, tables, target, window)
    bT, bc = ref.brute_table(pairs, sizes, tables, target, window)
    assert T.dtype == np.uint64 and T.shape == bT.shape and T.tobytes() == bT.tobytes() and counters.tolist() == bc.tolist()
    assert int(counters.sum()) == len(pairs[0]) and int(T.sum()) == int(counters[ref.ANCHORED])
    assert len(T) == ref.number_blocks(sizes, tables, target)[1]


def test_the_random_cases_hold_every_kind_of_pair():
    total = np.zeros(6, np.uint64)
    for seed in range(12):
        sizes, tables, target, pairs, window = _random_case(seed)
        total += ref.table(pairs, sizes, tables, target, window)[1]
    assert (total > 20).all(), total


def test_decisions_against_hand_worked_cases():
    B_ = [300, 200]
    pick = lambda a, size=50, mp=4, mr=2.0, ms=10: ref.choose_chromosome(a, B_, size, mp, mr, ms)
    assert pick([9, 1], size=5)[3] == "too_small" and pick([0, 0])[3] == "no_links"
    assert pick([3, 0]) == (0, 1, float("inf"), "ambiguous")                    # fewer than minPairs
    assert pick([6, 4])[3] == "ambiguous" and pick([6, 4])[:2] == (0, 1)        # 6 / 300 == 4 / 200: a tie, the lowest q first
    assert pick([6, 3]) == (0, 1, (6 * 200) / (3 * 300), "ambiguous")           # ratio 1.33
    assert pick([3, 6]) == (1, 0, (6 * 300) / (3 * 200), None)                  # ratio 3
    assert pick([6, 2]) == (0, 1, 2.0, None)                                    # ratio 2 is not below minRatio 2
    assert ref.choose_chromosome([7], [300], 50, 4, 2.0, 0) == (0, None, None, None)
    T = np.zeros((3, 2, 2), np.uint64)
    T[0, 0, ref.RIGHT], T[1, 1, ref.LEFT] = 5, 4
    assert ref.gap_scores(T, 1).tolist() == [[0, 0], [9, 0], [0, 0], [0, 0]]
    assert ref.gap_scores(T, 2).tolist() == [[4, 0], [9, 0], [5, 0], [0, 0]]
    assert ref.choose_gap(ref.gap_scores(T, 1), 4) == (1, "+", 9, 0, "placed") and ref.choose_gap(ref.gap_scores(T, 2), 4)[3] == 5
    assert ref.choose_gap(ref.gap_scores(T, 1), 10)[4] == "chromosome_only"
    T[0, 1, ref.RIGHT], T[1, 0, ref.LEFT] = 5, 4
    assert ref.choose_gap(ref.gap_scores(T, 1), 4) == (1, "+", 9, 9, "orientation_open")
    T[:] = 0
    T[0, 0, ref.RIGHT] = T[1, 0, ref.RIGHT] = 4
    assert ref.choose_gap(ref.gap_scores(T, 1), 4) == (1, "+", 4, 4, "chromosome_only")      # gaps 1 and 2 tie


# ---- anchor.h as host code under the sanitizers ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("anchor") / "anchor_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "anchor_host_check.cpp"), "-o", exe])

    def run(path, sizes, tables, target, window, pairs, print_table=True):
        seq, off, rev, seq_sizes = tables
        tgt = np.full(len(sizes), -1) if target is None else np.asarray(target)
        lines = ["T %d %d %d %d %d" % (len(sizes), len(seq_sizes), window, target is not None, print_table)]
        lines += ["%d %d %d %d %d" % row for row in zip(np.asarray(sizes).tolist(), seq.tolist(), off.tolist(), rev.tolist(), tgt.tolist())]
        lines += [" ".join(str(int(x)) for x in seq_sizes), "P %d" % len(pairs[0])]
        lines += ["%d %d %d %d" % row for row in zip(*(np.asarray(x).tolist() for x in pairs))]
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        # an ordinary child process, nothing preloaded
        done = subprocess.run([exe, path], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        return done.stdout.splitlines()
    return run


def _expected_lines(sizes, tables, target, window, pairs):
    first, n = ref.number_blocks(sizes, tables, target)
    kind, index = ref.classify(pairs, sizes, tables, target, window)
    T, counters = ref.table(pairs, sizes, tables, target, window)
    out = ["check 0 "] + (["targets 0 "] if target is not None else []) + ["table %d" % n] + ["first %d" % r for r in first]
    out += ["pair %d %d" % ki for ki in zip(kind.tolist(), index.tolist())]
    return out + ["counters " + " ".join(str(c) for c in counters.tolist())] + ["t %d" % c for c in T.tolist()]


@pytest.mark.parametrize("seed", range(12))
def test_native_blocks_kinds_and_table_under_the_sanitizers(seed, host_check, tmp_path):
    sizes, tables, target, pairs, window = _random_case(seed)
    assert host_check(str(tmp_path / "case.txt"), sizes, tables, target, window, pairs) == _expected_lines(sizes, tables, target, window, pairs)


def edge_pairs(sizes, tables, window):
    """Every candidate position 1, len - len / 2, len - len / 2 + 1 and len against both edges of both zones of every
    placed scaffold, in either mate order, and some pairs of the other kinds."""
    seq = tables[0]
    dropped = [s for s in range(len(sizes)) if seq[s] < 0 and sizes[s] > 0]
    placed = [s for s in range(len(sizes)) if seq[s] >= 0 and sizes[s] > 0]
    rows = []
    for k, c in enumerate(dropped):
        L = int(sizes[c])
        for pc in sorted({1, L - L // 2, min(L, L - L // 2 + 1), L}):
            for s in placed:
                M = int(sizes[s])
                wl, wr = min(window, M - M // 2), min(window, M // 2)
                for ps in sorted({1, wl, min(M, wl + 1), max(1, M - wr), M - wr + 1 if wr else M, M}):
                    rows.append((c, pc, s, ps) if (k + ps) % 2 else (s, ps, c, pc))
    rows += [(dropped[0], 1, dropped[1], 1), (dropped[2], 1, dropped[2], 1), (placed[0], 1, placed[1], 1)]
    return _pairs(rows)


@pytest.mark.parametrize("window", [1, 500, 10 ** 6])
def test_native_odd_scaffolds_halves_and_zone_edges_under_the_sanitizers(window, host_check, tmp_path):
    _names, sizes = bref.odd_scaffolds()
    assert sorted(set(sizes.tolist())) == [1, 999, 1000, 1001, 3007, 70000]
    tables = lref.layout(ODD_CHROMS, sizes, 100, drop_unplaced=True)
    assert tables[2].any() and not tables[2].all()                               # reversed scaffolds and forward ones
    pairs = edge_pairs(sizes, tables, window)
    got = host_check(str(tmp_path / "case.txt"), sizes, tables, None, window, pairs)
    assert got == _expected_lines(sizes, tables, None, window, pairs)
    # rank mode: the candidates in turn against Chr_1, Chr_2, Chr_3 and nothing; odd and even lengths have a target
    dropped = np.flatnonzero((tables[0] < 0)).tolist()
    target = np.full(40, -1, np.int32)
    for k, c in enumerate(dropped):
        target[c] = k % 4 - 1
    assert {int(sizes[c]) for c in dropped if target[c] >= 0} >= {1, 999, 1000, 1001, 3007}
    got = host_check(str(tmp_path / "case.txt"), sizes, tables, target, window, pairs)
    assert got == _expected_lines(sizes, tables, target, window, pairs)
    kinds = ref.table(pairs, sizes, tables, target, window)[1]
    assert (kinds[[ref.ANCHORED, ref.ELSEWHERE, ref.SKIPPED, ref.UNPLACED, ref.PLACED]] > 0).all() and (kinds[ref.MIDDLE] > 0) == (window < 10 ** 6)


def test_native_targets_are_refused_with_the_scaffold_named(host_check, tmp_path):
    tables = lref.layout(SMALL + [[(F, "+")]], SIZES, 100, drop_unplaced=True)   # Chr_3 holds the scaffold without a base alone
    none = _pairs([(0, 1, 0, 1)])
    for target, word in (([-1, 3, -1, -1, -1, -1], "scaffold 1 has the target 3, outside -1 .. 2"),
                         ([-1, -2, -1, -1, -1, -1], "scaffold 1 has the target -2, outside -1 .. 2"),
                         ([0, -1, -1, -1, -1, -1], "scaffold 0 has a target but lies in sequence 0"),
                         ([-1, -1, -1, -1, 2, -1], "scaffold 4 has the target 2, a sequence without a placed scaffold that has a base")):
        got = host_check(str(tmp_path / "case.txt"), SIZES, tables, target, 1, none)
        assert got == ["check 0 ", "targets -1 " + word]
    tables = lref.layout(SMALL, SIZES, 100, drop_unplaced=True)
    got = host_check(str(tmp_path / "case.txt"), SIZES, tables, [-1, -1, -1, -1, -1, 0], 1, none)
    assert got == ["check 0 ", "targets -1 scaffold 5 has a target but no base"]
    got = host_check(str(tmp_path / "case.txt"), SIZES, tables, [-1] * 6, 1, none)
    assert got[:3] == ["check 0 ", "targets 0 ", "table 0"]                      # no candidate


def test_native_table_limit_from_both_sides_under_the_sanitizers(host_check, tmp_path):
    none = _pairs([(0, 1, 0, 1)])
    # sequence mode: 2^13 sequences of one scaffold and 2^14 candidates fill 2^27 counters; one candidate more passes them
    n_seq = 2 ** 13
    for extra, fit in ((0, True), (1, False)):
        n = n_seq + 2 ** 14 + extra
        sizes = np.ones(n, np.int64)
        tables = lref.layout([[(q, "+")] for q in range(n_seq)], sizes, 0, drop_unplaced=True)
        got = host_check(str(tmp_path / "case.txt"), sizes, tables, None, 1, none, print_table=False)
        if fit:
            assert got[:2] == ["check 0 ", "table %d" % 2 ** 27] and got[2 + n_seq] == "first 0" and got[1 + n] == "first %d" % (2 ** 27 - n_seq)
            assert got[2 + n:] == ["pair %d -1" % ref.PLACED, "counters 0 0 0 0 0 1"]
        else:
            assert got == ["check 0 ", "table -1"]
    # rank mode: one sequence of 2^12 scaffolds, 2^13 candidates with it as their target
    S = 2 ** 12
    for extra, fit in ((0, True), (1, False)):
        n = S + 2 ** 13 + extra
        sizes = np.ones(n, np.int64)
        tables = lref.layout([[(s, "+") for s in range(S)]], sizes, 0, drop_unplaced=True)
        target = np.where(np.arange(n) < S, -1, 0)
        got = host_check(str(tmp_path / "case.txt"), sizes, tables, target, 1, none, print_table=False)
        assert got[:3] == ["check 0 ", "targets 0 ", "table %d" % (2 ** 27 if fit else -1)] and (len(got) > 3) == fit
        if fit:
            assert got[3 + S] == "first 0" and got[3 + S + 1] == "first %d" % (4 * S) and got[2 + n] == "first %d" % (2 ** 27 - 4 * S)


# ---- header, binding, switch ---------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_exports():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = re.sub(r"\s+", " ", fh.read())
    tables = "const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq"
    assert ("int hicmi_anchor_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, " + tables + ", const int32_t *target, "
            "int64_t window, int64_t *first_out, int64_t *n_table_out);") in text
    assert ("int hicmi_anchor_add_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b, "
            "const int64_t *pos_b, int64_t n);") in text
    assert "int hicmi_anchor_finish(hicmi_ctx *ctx, uint64_t *table_out, uint64_t *counters6_out);" in text
    assert ("int hicmi_anchor_file(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names, "
            "const int64_t *scaf_size, " + tables + ", const int32_t *target, int64_t window, hicmi_ctx *ctx, int threads, "
            "int64_t *stats5, uint64_t *table_out, uint64_t *counters6_out, int64_t *first_out, int64_t *n_table_out);") in text
    lib = _lib.load()
    for name, n_args in {"hicmi_anchor_begin": 12, "hicmi_anchor_add_pairs": 6, "hicmi_anchor_finish": 3, "hicmi_anchor_file": 19}.items():
        assert len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
        declared = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        assert declared.count(",") + 1 == n_args
    for method in ("anchor_begin", "anchor_add_pairs", "anchor_finish"):
        assert callable(getattr(_lib.Context, method))
    assert callable(_lib.anchor_file) and lib.hicmi_abi_version() == 1


def test_binding_blocks_equal_the_reference():
    from hic_genome_assembler_amd import _lib
    for seed in range(12):
        sizes, tables, target, _pairs_, _window = _random_case(seed)
        first, n = _lib.anchor_blocks(sizes, tables[0], len(tables[3]), target)
        want_first, want_n = ref.number_blocks(sizes, tables, target)
        assert first.dtype == np.int64 and first.tolist() == want_first.tolist() and n == want_n


def test_the_count_form_is_read_at_every_call_and_the_files_are_named():
    with open(os.path.join(CSRC, "api.hip")) as fh:
        api = fh.read()
    assert 'getenv("HICMI_ANCHOR_PLAIN")' in api and api.count("anchor_plain()") == 3      # a definition and two uses
    add = api[api.index("int hicmi_anchor_add_pairs("):api.index("int hicmi_anchor_finish(")]
    assert "anchor_plain()" in add
    for path in (os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))):
        with open(path) as fh:
            assert not [ln for ln in fh if "HICMI_ANCHOR_PLAIN" in ln and re.search(r"\bstatic\b[^;]*\bgetenv\(", ln)], path
    with open(os.path.join(CSRC, "hicmi_internal.h")) as fh:
        internal = fh.read()
    for name in ("ANCHOR_SLICE", "ANCHOR_SLOT_BITS", "ANCHOR_SLOTS", "ANCHOR_PROBES"):
        assert re.search(r"static constexpr int %s = " % name, internal), name
    with open(os.path.join(CSRC, "k_anchor.hip")) as fh:
        kernel = fh.read()
    assert "static_assert((ANCHOR_SLOTS & (ANCHOR_SLOTS - 1)) == 0" in kernel and "static_assert(ANCHOR_SLICE % 256 == 0" in kernel
    assert "static_assert(ANCHOR_MAX_TABLE <= (int64_t)1 << 31" in kernel
    with open(os.path.join(CSRC, "anchor.h")) as fh:
        includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", fh.read())
    assert includes == ['"ends.h"']                                                          # no GPU dependency
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    assert " anchor.h " in make and " k_anchor.hip " in make
    with open(os.path.join(ROOT, "README.md")) as fh:
        readme = fh.read()
    for word in ("placeUnplaced", "HICMI_ANCHOR_PLAIN", "k_anchor.hip", "anchor.h", "unplacedSupport.txt", "choices, not tuned values"):
        assert word in readme, word
    # the anchor calls are not readers of the contact matrix, of a map build, of a span build or of an ends build
    code = api[api.index("static void anchor_abandon"):api.index("// Group support (DESIGN.md 9f)")]
    assert "hicmi_anchor_file(" in code
    for word in ("c->dC", "map_cells", "drop_matrix_state", "span_marks", "span_grid", "map_m", "ends_table", "ends_grid", "ends_cells"):
        assert word not in code, word


# ---- the command line on a stand-in context ------------------------------------------------------------------------------------------
class StandInContext:
    """The array calls of _lib.Context, answered by the reference."""

    def __init__(self):
        self.calls, self.open = [], None

    def anchor_begin(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window):
        tables = (np.asarray(lift_seq, np.int32), np.asarray(lift_off, np.int64), np.asarray(lift_rev, np.uint8), np.asarray(seq_sizes, np.int64))
        self.open = (np.asarray(sizes, np.int64), tables, None if target is None else np.asarray(target, np.int32), int(window), [])
        self.calls.append(("rank" if target is not None else "sequence", int(window)))
        return ref.number_blocks(self.open[0], tables, self.open[2])[0]

    def anchor_add_pairs(self, sa, pa, sb, pb):
        self.open[4].append((sa, pa, sb, pb))

    def anchor_finish(self):
        sizes, tables, target, window, parts = self.open
        self.open = None
        pairs = tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
        return ref.table(pairs, sizes, tables, target, window)


def _read(path):
    with open(path, newline="") as fh:
        return fh.read()


def _case_files(tmp_path, names, sizes, order_text, pairs):
    from hic_genome_assembler_amd import synth
    d = str(tmp_path)
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    with open(paths["hicProScaffSizeFile"], "w") as fh:
        fh.write("".join("%s\t%d\n" % ns for ns in zip(names, np.asarray(sizes).tolist())))
    pair_file = os.path.join(d, "case.allValidPairs")
    with open(pair_file, "wb") as fh:
        fh.write(ref.pair_file_bytes(names, pairs))
    order = os.path.join(d, "orders.txt")
    with open(order, "w", newline="") as fh:
        fh.write(order_text)
    save = os.path.join(d, "save")
    cfg = synth.write_config(os.path.join(d, "config.txt"), paths, save, os.path.join(d, "plots"), 100000, extra={"validPairFile": pair_file})
    return cfg, order, save, paths


def _ratio_text(ratio):
    return "NA" if ratio is None else "inf" if ratio == float("inf") else "%.6g" % ratio


def expected_report(names, sizes, chroms, pairs, window, reach, min_pairs, min_ratio, min_size, n_lines=None):
    """(report text, the winners {(chromosome, gap): candidate}, the reference's result) from the reference."""
    result, winners, counters1, counters2 = ref.place(sizes, chroms, pairs, window, reach, min_pairs, min_ratio, min_size)
    n_pairs = len(pairs[0])
    head = "#window=%d\treach=%d\tminPairs=%d\tminRatio=%g\tminSize=%d\tlines=%d\tused=%d\tunknown_scaffold=0\tout_of_range=0" % (
        window, reach, min_pairs, min_ratio, min_size, n_pairs if n_lines is None else n_lines, n_pairs)
    head += "".join("\tchromosomes_%s=%d" % kv for kv in zip(ref.COUNTERS, counters1.tolist()))
    head += "".join("\tgaps_%s=%d" % kv for kv in zip(ref.COUNTERS, counters2.tolist()))
    out = [head, "### Unplaced ###", "#scaffold\tsize\tlinks\tchromosome\tchrom_links\tsecond\tsecond_links\tratio\tleft\tright\torientation\t"
                                     "score\trunner_up\tverdict"]
    filled = [[s for s, _o in ch if sizes[s] > 0] for ch in chroms]
    for c in sorted(result):
        r = result[c]
        a, linked = r["links"], sum(r["links"]) > 0
        cols = [names[c], "%d" % sizes[c], "%d" % sum(a)]
        cols += ["%d" % (r["best"] + 1), "%d" % a[r["best"]]] if linked else ["NA", "NA"]
        cols += ["%d" % (r["second"] + 1), "%d" % a[r["second"]]] if linked and r["second"] is not None else ["NA", "NA"]
        cols.append(_ratio_text(r["ratio"] if linked else None))
        if r["gap"] is None:
            cols += ["NA"] * 5
        else:
            members, g = filled[r["best"]], r["gap"]
            if r["verdict"] == "chromosome_only":
                cols += ["NA"] * 3
            else:
                cols += [names[members[g - 1]] if g else "start", names[members[g]] if g < len(members) else "end", r["orientation"]]
            cols += ["%d" % r["score"], "%d" % r["runner_up"]]
        out.append("\t".join(cols + [r["verdict"]]))
    out += ["### Chromosomes ###", "#chromosome\tscaffolds\tbases\tassigned\tinserted"]
    for q in range(len(chroms)):
        out.append("%d\t%d\t%d\t%d\t%d" % (q + 1, len(filled[q]), sum(int(sizes[s]) for s in filled[q]),
                                           sum(r["gap"] is not None and r["best"] == q for r in result.values()),
                                           sum(key[0] == q for key in winners)))
    return "\n".join(out) + "\n", winners, result


# Chr_1 = p1+ z0 p2- p3+ z1 (z0, z1 without a base), Chr_2 = r1+ r2+; the placed scaffolds have 100 bases, the window is 10
V_NAMES = ["p1", "z0", "p2", "p3", "z1", "r1", "r2", "t_small", "nolinks", "amb_pairs", "amb_ratio", "amb_tie", "co_pairs", "co_tie",
           "plus", "minus", "last", "open", "late", "last_too"]
V_SIZES = np.array([100, 0, 100, 100, 0, 100, 100, 5] + [50] * 12, dtype=np.int64)
V_CHROMS = [[(0, "+"), (1, "+"), (2, "-"), (3, "+"), (4, "+")], [(5, "+"), (6, "+")]]
V_ORDER = ("### Chromosome grouping 1 ###\r\np1\t+\r\nz0\t+\r\np2\t-\tnote\r\np3\t+\r\nz1\t+\r\n"
           "### Chromosome grouping 2 ###\nr1\t+\nr2\t+")
V_WINDOW, V_MIN_PAIRS, V_MIN_RATIO, V_MIN_SIZE = 10, 4, 2.0, 10


def _verdict_pairs():
    ix = {n: k for k, n in enumerate(V_NAMES)}
    reversed_ = {"p2"}

    def zone(s, which):                                             # a position in the LEFT (0), RIGHT (1) zone or the middle (2) as s lies
        x = {0: 3, 1: 96, 2: 50}[which]                            # lying coordinate, 0-based
        return 100 - x if s in reversed_ else x + 1

    def link(c, half, s, which, n):
        return [(ix[c], 10 if half == 0 else 40, ix[s], zone(s, which))] * n

    rows = link("t_small", 0, "p1", 1, 9)[:0] + [(ix["t_small"], 2, ix["p1"], 50)] * 9
    rows += link("amb_pairs", 0, "p1", 2, 3)
    rows += link("amb_ratio", 0, "p1", 2, 6) + link("amb_ratio", 0, "r1", 2, 3)
    rows += link("amb_tie", 0, "p3", 2, 6) + link("amb_tie", 1, "r2", 2, 4)
    rows += link("co_pairs", 0, "p2", 2, 5) + link("co_pairs", 0, "p2", 1, 3)
    rows += link("co_tie", 0, "p1", 1, 4) + link("co_tie", 0, "p2", 1, 4)
    rows += link("plus", 0, "p1", 1, 5) + link("plus", 1, "p2", 0, 5) + link("plus", 1, "r1", 2, 1)
    rows += link("minus", 0, "r1", 0, 6)                            # its first half faces r1's left end: it lies reversed before r1
    rows += link("last", 0, "p3", 1, 5)
    rows += link("open", 0, "p2", 1, 4) + link("open", 1, "p2", 1, 4)
    rows += link("late", 0, "p1", 1, 4)                             # gap 1 of Chr_1 like plus, with 4 against 10
    rows += link("last_too", 0, "p3", 1, 5)                         # gap 3 of Chr_1 like last, with the same score
    rows += [(ix["p1"], 5, ix["p3"], 7), (ix["plus"], 1, ix["minus"], 1), (ix["nolinks"], 1, ix["nolinks"], 9)]
    return _pairs(rows)


V_VERDICTS = {"t_small": "too_small", "nolinks": "no_links", "amb_pairs": "ambiguous", "amb_ratio": "ambiguous", "amb_tie": "ambiguous",
              "co_pairs": "chromosome_only", "co_tie": "chromosome_only", "plus": "placed", "minus": "placed", "last": "placed",
              "open": "orientation_open", "late": "deferred", "last_too": "deferred"}


def test_cli_every_verdict_on_a_stand_in_context(tmp_path, capsys):
    from hic_genome_assembler_amd import placeUnplaced
    from hic_genome_assembler_amd.assembledMap import build_assembly, read_order_file
    pairs = _verdict_pairs()
    cfg, order, save, _paths = _case_files(tmp_path, V_NAMES, V_SIZES, V_ORDER, pairs)
    ctx = StandInContext()
    placed, full = str(tmp_path / "placed.txt"), str(tmp_path / "full")
    args = ["-config", cfg, "-order", order, "-window", "%d" % V_WINDOW, "-reach", "1", "-minSize", "%d" % V_MIN_SIZE, "-placed", placed,
            "-full", full, "-threads", "2"]
    _stats, verdicts, inserted = placeUnplaced.main(args, context=ctx)
    assert ctx.calls == [("sequence", V_WINDOW), ("rank", V_WINDOW)] and ctx.open is None
    assert {V_NAMES[s]: x for s, x in verdicts.items()} == V_VERDICTS
    want, winners, result = expected_report(V_NAMES, V_SIZES, V_CHROMS, pairs, V_WINDOW, 1, V_MIN_PAIRS, V_MIN_RATIO, V_MIN_SIZE)
    report = _read(os.path.join(save, "unplacedSupport.txt"))
    assert report == want
    assert {V_NAMES[c]: key for key, c in winners.items()} == {"plus": (0, 1), "minus": (1, 0), "last": (0, 3), "open": (0, 2)}
    assert inserted == {"plus": (0, 1, "+"), "minus": (1, 0, "-"), "last": (0, 3, "+"), "open": (0, 2, "+")}
    lines = {ln.split("\t")[0]: ln.split("\t") for ln in report.splitlines()[3:3 + 13]}
    assert lines["plus"] == ["plus", "50", "11", "1", "10", "2", "1", "%.6g" % ((10 * 200) / (1 * 300)), "p1", "p2", "+", "10", "0", "placed"]
    assert lines["minus"][8:] == ["start", "r1", "-", "6", "0", "placed"] and lines["last"][8:] == ["p3", "end", "+", "5", "0", "placed"]
    assert lines["open"][8:] == ["p2", "p3", "+", "4", "4", "orientation_open"] and lines["late"][8:] == ["p1", "p2", "+", "4", "0", "deferred"]
    assert lines["co_tie"][8:] == ["NA", "NA", "NA", "4", "4", "chromosome_only"] and lines["nolinks"][2:] == ["0"] + ["NA"] * 10 + ["no_links"]
    assert lines["amb_tie"][3:8] == ["1", "6", "2", "4", "1"] and lines["t_small"][2:8] == ["9", "1", "9", "2", "0", "inf"]
    assert report.splitlines()[-2:] == ["1\t3\t300\t7\t3", "2\t2\t200\t1\t1"]
    # the order file again: CR LF lines keep their ending, the line after a scaffold without a base, the last line without an ending
    text = _read(placed)
    assert text == ("### Chromosome grouping 1 ###\r\np1\t+\r\nz0\t+\r\nplus\t+\r\np2\t-\tnote\r\nopen\t+\r\np3\t+\r\nlast\t+\r\nz1\t+\r\n"
                    "### Chromosome grouping 2 ###\nminus\t-\nr1\t+\nr2\t+")
    assert text == ref.placed_text(V_ORDER, V_NAMES, V_SIZES, V_CHROMS, result, winners) and _read(order) == V_ORDER
    asm = build_assembly(read_order_file(placed), V_NAMES, V_SIZES, 100, chromosomes_only=True)
    assert [[V_NAMES[s] for s, _off, _o in comps] for comps in asm.components] == [["p1", "z0", "plus", "p2", "open", "p3", "last", "z1"],
                                                                                   ["minus", "r1", "r2"]]
    chrom_rows = _read(os.path.join(full, "unplaced.chromosomes.tsv")).splitlines()
    assert chrom_rows[0] == "#scaffold\tChr_1\tChr_2" and chrom_rows[1:] == ["%s\t%d\t%d" % ((V_NAMES[c],) + tuple(result[c]["links"])) for c in sorted(result)]
    gap_rows = _read(os.path.join(full, "unplaced.gaps.tsv")).splitlines()
    want_rows = []
    for c in sorted(result):
        if result[c]["gap"] is not None:
            members = [V_NAMES[s] for s, _o in V_CHROMS[result[c]["best"]] if V_SIZES[s] > 0]
            for g in range(len(members) + 1):
                for o in (0, 1):
                    want_rows.append("%s\t%d\t%d\t%s\t%s\t%s\t%d" % (V_NAMES[c], result[c]["best"] + 1, g, members[g - 1] if g else "start",
                                                                    members[g] if g < len(members) else "end", "+-"[o], result[c]["scores"][g, o]))
    assert gap_rows[0] == "#scaffold\tchromosome\tgap\tleft\tright\torientation\tscore" and gap_rows[1:] == want_rows
    assert "UNPLACED: 13 unplaced scaffold(s), 8 with a chromosome, 4 inserted, 2 deferred" in capsys.readouterr().out
    # a second run on the placed file places the deferred ones next to the winners
    out2, placed2 = str(tmp_path / "second.txt"), str(tmp_path / "placed2.txt")
    _stats, verdicts2, inserted2 = placeUnplaced.main(["-config", cfg, "-order", placed, "-window", "%d" % V_WINDOW, "-reach", "1", "-minSize",
                                                       "%d" % V_MIN_SIZE, "-out", out2, "-placed", placed2], context=StandInContext())
    assert set(inserted2) >= {"last_too"} and "late" in {V_NAMES[s] for s in verdicts2}


@pytest.mark.parametrize("reach", [2, 64])
def test_cli_report_equals_the_reference_at_other_reaches_and_through_an_anchor_file_context(reach, tmp_path):
    from hic_genome_assembler_amd import placeUnplaced
    pairs = _verdict_pairs()
    cfg, order, save, _paths = _case_files(tmp_path, V_NAMES, V_SIZES, V_ORDER, pairs)

    class FileContext:
        def anchor_file(self, path, names, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window, threads=0):
            with open(path, "rb") as fh:
                got, stats, _after = bref.parse_text(fh.read(), names, sizes)
            tables = (np.asarray(lift_seq, np.int32), np.asarray(lift_off, np.int64), np.asarray(lift_rev, np.uint8), np.asarray(seq_sizes, np.int64))
            return (stats + (1,), ref.number_blocks(sizes, tables, target)[0]) + ref.table(got, sizes, tables, target, window)

    for k, context in enumerate((StandInContext(), FileContext())):
        out = str(tmp_path / ("report%d.txt" % k))
        placeUnplaced.main(["-config", cfg, "-order", order, "-window", "%d" % V_WINDOW, "-reach", "%d" % reach, "-out", out], context=context)
        assert _read(out) == expected_report(V_NAMES, V_SIZES, V_CHROMS, pairs, V_WINDOW, reach, 4, 2.0, 0)[0]
    assert os.listdir(str(tmp_path / "save")) == [] if os.path.isdir(str(tmp_path / "save")) else True


def test_placed_text_line_endings():
    from hic_genome_assembler_amd import placeUnplaced
    import tempfile
    names, sizes = ["a", "b", "x", "y"], np.array([5, 5, 5, 5])
    chroms = [[(0, "+"), (1, "-")]]
    result = {2: {"orientation": "-"}, 3: {"orientation": "+"}}
    for text in ("### 1 ###\na\t+\nb\t-", "### 1 ###\r\na\t+\r\nb\t-\r\n", "### 1 ###\na\t+\r\nb\t-\n"):
        for winners in ({(0, 2): 2}, {(0, 0): 3, (0, 2): 2}, {(0, 1): 3}):
            with tempfile.TemporaryDirectory() as d:
                path = os.path.join(d, "o.txt")
                with open(path, "w", newline="") as fh:
                    fh.write(text)
                ins = {}
                for (q, g), c in winners.items():
                    ins[names[g] if g < 2 else ("b", None)] = (names[c], result[c]["orientation"])
                got = placeUnplaced.placed_order_text(path, ins)
            assert got == ref.placed_text(text, names, sizes, chroms, result, winners)
            assert got.count("\n") == text.count("\n") + len(winners) and got.replace("x\t-", "").replace("y\t+", "").count("\t") == 2
    assert ref.placed_text("### 1 ###\na\t+\nb\t-", names, sizes, chroms, result, {(0, 2): 2}) == "### 1 ###\na\t+\nb\t-\nx\t-"
    assert ref.placed_text("### 1 ###\na\t+\r\nb\t-\n", names, sizes, chroms, result, {(0, 0): 3}) == "### 1 ###\ny\t+\r\na\t+\r\nb\t-\n"


def test_nothing_is_unplaced(tmp_path, capsys):
    from hic_genome_assembler_amd import placeUnplaced
    names, sizes = ["a", "b", "c"], np.array([10, 0, 10])
    pairs = _pairs([(0, 1, 2, 1)])
    text = "### 1 ###\na\t+\nc\t-\n"                                    # b has no base: it is not a candidate
    cfg, order, save, _paths = _case_files(tmp_path, names, sizes, text, pairs)
    ctx = StandInContext()
    placed = str(tmp_path / "placed.txt")
    placeUnplaced.main(["-config", cfg, "-order", order, "-placed", placed], context=ctx)
    assert ctx.calls == [] and "nothing is unplaced" in capsys.readouterr().out
    report = _read(os.path.join(save, "unplacedSupport.txt")).splitlines()
    assert report[1:] == ["### Unplaced ###", "#" + "\t".join(placeUnplaced.UNPLACED_COLUMNS), "### Chromosomes ###",
                          "#" + "\t".join(placeUnplaced.CHROMOSOME_COLUMNS), "1\t2\t20\t0\t0"]
    assert _read(placed) == text


def test_bad_input_is_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import placeUnplaced, synth
    pairs = _verdict_pairs()
    cfg, order, save, paths = _case_files(tmp_path, V_NAMES, V_SIZES, V_ORDER, pairs)
    d = str(tmp_path)
    out = os.path.join(d, "report.txt")
    ctx = StandInContext()

    def write(text, name):
        path = os.path.join(d, name)
        with open(path, "w") as fh:
            fh.write(text)
        return path

    def refused(word, more=(), config=cfg, order_file=order, context=ctx):
        args = ["-config", config, "-out", out, "-placed", out + ".placed", "-full", out + ".full"] + (["-order", order_file] if order_file else [])
        with pytest.raises(SystemExit) as exc:
            placeUnplaced.main(args + list(more), context=context)
        assert word in str(exc.value.code) and str(exc.value.code).startswith("ERROR... ") and \
            str(exc.value.code).endswith(" Exiting..."), exc.value.code

    refused("window", ["-window", "0"])
    refused("window", ["-window", "-5"])
    refused("reach", ["-reach", "0"])
    refused("reach", ["-reach", "65"])
    refused("minPairs", ["-minPairs", "-1"])
    refused("minSize", ["-minSize", "-1"])
    refused("minRatio", ["-minRatio", "0.99"])
    refused("minRatio", ["-minRatio", "nan"])
    refused("zz", order_file=write("### 1 ###\np1\t+\nzz\t+\n", "unknown.txt"))
    refused("twice", order_file=write("### 1 ###\np1\t+\n### 2 ###\np2\t+\np1\t-\n", "twice.txt"))
    refused("orientation", order_file=write("### 1 ###\np1\t+\np2\t?\n", "orient.txt"))
    refused("no scaffold", order_file=write("### 1 ###\np1\t+\n### 2 ###\n", "empty.txt"))
    refused("orientation column", order_file=write("### 1 ###\np1\n", "one_column.txt"))
    refused("does not exist", order_file=os.path.join(d, "nothing_here"))
    refused("does not exist", order_file=None)                               # neither default order file is there
    assert ctx.calls == []
    # pass 1: 2^14 + 1 unplaced scaffolds against 2^13 chromosomes, one block past the table
    n_seq, n = 2 ** 13, 2 ** 13 + 2 ** 14 + 1
    big = dict(paths, hicProScaffSizeFile=write("".join("s%d\t1\n" % k for k in range(n)), "big.sizes"))
    big_cfg = synth.write_config(os.path.join(d, "big.txt"), big, save, os.path.join(d, "plots"), 100000,
                                 extra={"validPairFile": os.path.join(d, "case.allValidPairs")})
    big_order = write("".join("### %d ###\ns%d\t+\n" % (k, k) for k in range(n_seq)), "big.order")
    refused("-minSize", config=big_cfg, order_file=big_order)
    refused("%d counters" % ((2 ** 14 + 1) * n_seq), config=big_cfg, order_file=big_order)
    assert ctx.calls == []
    # pass 2: 2^13 + 1 scaffolds that get the one chromosome of 2^12 scaffolds: 4 x 2^12 counters each
    S, n = 2 ** 12, 2 ** 12 + 2 ** 13 + 1
    names = ["s%d" % k for k in range(n)]
    wide = dict(paths, hicProScaffSizeFile=write("".join("%s\t1\n" % x for x in names), "wide.sizes"))
    wide_pairs = write("".join("r\t%s\t1\t+\ts0\t1\t-\n" % names[k] for k in range(S, n)), "wide.pairs")
    wide_cfg = synth.write_config(os.path.join(d, "wide.txt"), wide, save, os.path.join(d, "plots"), 100000, extra={"validPairFile": wide_pairs})
    wide_order = write("### 1 ###\n" + "".join("%s\t+\n" % x for x in names[:S]), "wide.order")

    class CountsOnly:                                                        # answers pass 1 as the reference would, without its loops
        calls = 0

        def anchor_file(self, path, names_, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window, threads=0):
            CountsOnly.calls += 1
            assert target is None
            first = np.where(np.arange(n) >= S, np.arange(n) - S, -1).astype(np.int64)
            return (n - S, n - S, 0, 0, 1), first, np.ones(n - S, np.uint64), np.array([n - S, 0, 0, 0, 0, 0], np.uint64)

    refused("raise -minSize", ["-minPairs", "1"], config=wide_cfg, order_file=wide_order, context=CountsOnly())
    assert CountsOnly.calls == 1
    refused("validPairFile", config=synth.write_config(os.path.join(d, "c2.txt"), paths, save, os.path.join(d, "plots"), 100000))
    missing = synth.write_config(os.path.join(d, "c3.txt"), paths, save, os.path.join(d, "plots"), 100000,
                                 extra={"validPairFile": os.path.join(d, "no_such_pairs")})
    refused("validPairFile", config=missing)
    assert os.listdir(save) == []
    assert not any(os.path.exists(p) for p in (out, out + ".placed", out + ".full"))


# ---- the planted case on the reference alone ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_rounds():
    """(P, round 1 = (result, winners), the chromosomes after round 1, round 2 = (result, winners))."""
    P = ref.planted()
    r1 = ref.place(P["sizes"], P["chroms"], P["pairs"], ref.PLANTED_WINDOW, ref.PLANTED_REACH, ref.PLANTED_MIN_PAIRS, ref.PLANTED_MIN_RATIO, 0)[:2]
    chroms = [list(ch) for ch in P["chroms"]]
    for (q, g), c in sorted(r1[1].items(), key=lambda kv: -kv[0][1]):       # from the back, so that the gaps before stay where they are
        chroms[q].insert(g, (c, r1[0][c]["orientation"]))
    r2 = ref.place(P["sizes"], chroms, P["pairs"], ref.PLANTED_WINDOW, ref.PLANTED_REACH, ref.PLANTED_MIN_PAIRS, ref.PLANTED_MIN_RATIO, 0)[:2]
    return P, r1, chroms, r2


def test_planted_scaffolds_return_on_the_reference_alone():
    """40 scaffolds in three chromosomes, eight taken out of the order file (6.2 to 40 kb; scaf_1 a chromosome's first,
    scaf_14, scaf_27 and scaf_40 its last; + and - ones): every one goes back to its chromosome (density ratios 14 to 56),
    its gap and its orientation; scaf_30 and scaf_31 belong in one gap, so scaf_30 (52 against 109) is deferred and returns in
    a second round.  The smallest margin of a score over its runner-up is 5 (scaf_30 in round 1: 52 against 47)."""
    P, (result, winners), chroms, (result2, winners2) = planted_rounds()
    truth = ref.planted_truth(P)
    assert sorted(result) == P["removed"] and {o for _q, _g, o in truth.values()} == {"+", "-"}
    assert min(P["sizes"][P["removed"]]) < 2 * ref.PLANTED_WINDOW < max(P["sizes"][P["removed"]])
    for c, r in result.items():
        assert (r["best"], r["gap"], r["orientation"]) == truth[c], (c, r)
        assert r["ratio"] > 10 and r["score"] - r["runner_up"] >= 5
    assert {c: r["verdict"] for c, r in result.items()} == {c: "deferred" if c == 29 else "placed" for c in P["removed"]}
    assert sorted(winners.values()) == [c for c in P["removed"] if c != 29]
    truth2 = ref.planted_truth(P, chroms)
    assert sorted(result2) == [29] and (result2[29]["best"], result2[29]["gap"], result2[29]["orientation"]) == truth2[29]
    assert result2[29]["verdict"] == "placed" and winners2 == {(2, 2): 29}
    chroms[2].insert(2, (29, result2[29]["orientation"]))
    assert chroms == P["true_chroms"]
