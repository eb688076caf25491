"""The resident pair store without a GPU: csrc/pairs.h built as host code with the sanitizers and compared
line by line with tests/pairs_reference.py, the tables of 9p and 9q from (kept pairs, intra) against the references on all
pairs, and the declarations.  Every comparison is exact."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import anchor_reference as aref
import ends_reference as eref
import liftmap_reference as lref
import pairs_reference as ref
import test_anchor_cpu as anchor_cases
import test_ends_cpu as ends_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")


def _pairs(rows):
    sa, pa, sb, pb = zip(*rows)
    return (np.array(sa, np.int32), np.array(pa, np.int64), np.array(sb, np.int32), np.array(pb, np.int64))


# ---- pairs.h as host code under the sanitizers --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pairs") / "pairs_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "pairs_host_check.cpp"), "-o", exe])

    def run(path, lift_seq, pairs, first):
        lines = ["S %d" % len(lift_seq), " ".join(str(int(q)) for q in lift_seq), "P %d %d" % (len(pairs[0]), first)]
        lines += ["%d %d %d %d" % row for row in zip(*(np.asarray(x).tolist() for x in pairs))]
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        # an ordinary child process, nothing preloaded
        done = subprocess.run([exe, path], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        return done.stdout.splitlines()
    return run


def _expected_lines(lift_seq, pairs):
    kept, counts = ref.keep(pairs), ref.intra(pairs, len(lift_seq))
    placed, dropped = ref.intra_sums(counts, lift_seq)
    out = ["keep %d" % k for k in ref.mask(pairs).tolist()] + ["kept %d" % len(kept[0])]
    out += ["k %d %d %d %d" % row for row in zip(*(x.tolist() for x in kept))] + ["intra %d" % c for c in counts.tolist()]
    out.append("sums %d %d" % (placed, dropped))
    out.append("ends 1 2 %d 4 5 %d" % (3 + placed, 6 + dropped))          # same, unlifted
    out.append("anchor 1 2 3 4 %d %d" % (5 + dropped, 6 + placed))        # unplaced, placed
    return out


@pytest.mark.parametrize("seed", range(12))
def test_native_mask_intra_and_sums_under_the_sanitizers(seed, host_check, tmp_path):
    sizes, tables, pairs, _window, _reach = ends_cases._random_case(seed)
    n = len(pairs[0])
    assert 0 < int(ref.mask(pairs).sum()) < n
    for first in (0, n // 3, n):
        assert host_check(str(tmp_path / "case.txt"), tables[0], pairs, first) == _expected_lines(tables[0], pairs)


def test_native_hand_worked_case_under_the_sanitizers(host_check, tmp_path):
    # scaffolds 0 and 1 placed, 2 dropped; the store keeps rows 0, 3 and 5 in this order
    pairs = _pairs([(0, 1, 1, 2), (0, 3, 0, 4), (2, 1, 2, 1), (2, 5, 0, 1), (1, 1, 1, 9), (1, 2, 2, 2), (2, 7, 2, 8)])
    got = host_check(str(tmp_path / "case.txt"), [0, 0, -1], pairs, 4)
    assert got == _expected_lines([0, 0, -1], pairs)
    assert got[:8] == ["keep 1", "keep 0", "keep 0", "keep 1", "keep 0", "keep 1", "keep 0", "kept 3"]
    assert got[8:11] == ["k 0 1 1 2", "k 2 5 0 1", "k 1 2 2 2"] and got[11:14] == ["intra 1", "intra 1", "intra 2"]
    assert got[14:] == ["sums 2 2", "ends 1 2 5 4 5 8", "anchor 1 2 3 4 7 8"]


def test_native_positions_above_2_to_the_32_under_the_sanitizers(host_check, tmp_path):
    big = [2 ** 32 + 1, 2 ** 33, 2 ** 62 - 5, 1, 2 ** 31, 2 ** 32 - 1]
    pairs = _pairs([(a % 3, p, b % 3, q) for a, p in enumerate(big) for b, q in enumerate(big)])
    got = host_check(str(tmp_path / "case.txt"), [0, -1, 1], pairs, 7)
    assert got == _expected_lines([0, -1, 1], pairs)
    assert "k 0 %d 1 %d" % (2 ** 32 + 1, 2 ** 33) in got and "k 2 %d 0 %d" % (2 ** 62 - 5, 1) in got


def test_native_none_kept_all_kept_and_no_pair_under_the_sanitizers(host_check, tmp_path):
    for rows in ([(1, 1, 1, 2)] * 5, [(0, 1, 1, 2)] * 5):
        assert host_check(str(tmp_path / "case.txt"), [0, 0], _pairs(rows), 2) == _expected_lines([0, 0], _pairs(rows))
    none = tuple(np.zeros(0, t) for t in (np.int32, np.int64, np.int32, np.int64))
    assert host_check(str(tmp_path / "case.txt"), [0, -1], none, 0) == ["kept 0", "intra 0", "intra 0", "sums 0 0", "ends 1 2 3 4 5 6",
                                                                       "anchor 1 2 3 4 5 6"]


# ---- the tables from the store equal the tables from all pairs ----------------------------------------------------------------
@pytest.mark.parametrize("seed", range(12))
def test_ends_table_from_the_store_equals_the_reference_on_all_pairs(seed):
    sizes, tables, pairs, window, reach = ends_cases._random_case(seed)
    kept, counts = ref.keep(pairs), ref.intra(pairs, len(sizes))
    assert len(kept[0]) + int(counts.sum()) == len(pairs[0]) and int(counts.sum()) > 0
    for W, R in ((window, reach), (1, 1), (1000, 64)):
        T, counters = ref.ends_table(kept, counts, sizes, tables, W, R)
        wT, wc = eref.table(pairs, sizes, tables, W, R)
        assert T.tobytes() == wT.tobytes() and counters.tolist() == wc.tolist()


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", [0, 100])
def test_ends_table_from_the_store_on_the_hand_worked_assembly(gap, drop):
    sizes, chroms = ends_cases.SIZES, ends_cases.CHROMS
    tables = lref.layout(chroms, sizes, gap, drop_unplaced=drop)
    ends = [(s, p) for s in range(5) for p in range(1, int(sizes[s]) + 1)]
    pairs = _pairs([a + b for a in ends for b in ends])
    kept, counts = ref.keep(pairs), ref.intra(pairs, len(sizes))
    assert counts.tolist() == [25, 1, 49, 9, 16, 0]
    for window in (1, 2, 3, 100):
        for reach in (1, 2, 64):
            T, counters = ref.ends_table(kept, counts, sizes, tables, window, reach)
            wT, wc = eref.table(pairs, sizes, tables, window, reach)
            assert T.tobytes() == wT.tobytes() and counters.tolist() == wc.tolist()
    # the intra pairs of e are unlifted when e is dropped and same when it is a sequence of its own
    assert int(wc[eref.SAME]) == 25 + 1 + 49 + 9 + (0 if drop else 16)


@pytest.mark.parametrize("seed", range(12))
def test_anchor_table_from_the_store_equals_the_reference_on_all_pairs_in_both_modes(seed):
    sizes, tables, target, pairs, window = anchor_cases._random_case(seed)
    kept, counts = ref.keep(pairs), ref.intra(pairs, len(sizes))
    assert int(counts.sum()) > 0
    for W in (window, 1, 1000):
        T, counters = ref.anchor_table(kept, counts, sizes, tables, target, W)
        wT, wc = aref.table(pairs, sizes, tables, target, W)
        assert T.tobytes() == wT.tobytes() and counters.tolist() == wc.tolist()


def test_the_random_cases_cover_both_anchor_modes_and_drop_on_and_off():
    assert {anchor_cases._random_case(seed)[2] is None for seed in range(12)} == {True, False}
    assert {bool((ends_cases._random_case(seed)[1][0] < 0).any()) for seed in range(12)} == {True, False}


# ---- header, binding, switch -------------------------------------------------------------------------------------------------
EXPORTS = {"hicmi_pairs_begin": 3, "hicmi_pairs_add": 6, "hicmi_pairs_file": 8, "hicmi_pairs_info": 4, "hicmi_pairs_fetch": 5,
           "hicmi_pairs_drop": 1, "hicmi_ends_resident": 14, "hicmi_anchor_resident": 14}


def test_header_and_binding_declare_the_exports():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = re.sub(r"\s+", " ", fh.read())
    tables = "const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq"
    assert "int hicmi_pairs_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf);" in text
    assert ("int hicmi_pairs_add(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b, "
            "const int64_t *pos_b, int64_t n);") in text
    assert ("int hicmi_pairs_file(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names, "
            "const int64_t *scaf_size, hicmi_ctx *ctx, int threads, int64_t *stats5);") in text
    assert "int hicmi_pairs_info(hicmi_ctx *ctx, int64_t *n_kept_out, uint64_t *n_intra_out, uint64_t *intra_out);" in text
    assert "int hicmi_pairs_fetch(hicmi_ctx *ctx, int32_t *scaf_a, int64_t *pos_a, int32_t *scaf_b, int64_t *pos_b);" in text
    assert "int hicmi_pairs_drop(hicmi_ctx *ctx);" in text
    assert ("int hicmi_ends_resident(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, " + tables + ", int64_t window, "
            "int64_t reach, uint64_t *table_out, uint64_t *counters6_out, int32_t *rank_out, int64_t *n_placed_out);") in text
    assert ("int hicmi_anchor_resident(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, " + tables + ", const int32_t *target, "
            "int64_t window, uint64_t *table_out, uint64_t *counters6_out, int64_t *first_out, int64_t *n_table_out);") in text
    lib = _lib.load()
    for name, n_args in EXPORTS.items():
        assert len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
        declared = re.search(r"int %s\(([^;]*)\);" % name, text).group(1)
        assert declared.count(",") + 1 == n_args
    for method in ("pairs_begin", "pairs_add", "pairs_info", "pairs_fetch", "pairs_drop", "pairs_file", "ends_resident", "anchor_resident"):
        assert callable(getattr(_lib.Context, method))
    assert callable(_lib.pairs_file) and lib.hicmi_abi_version() == 1
    assert set(_lib.SIGNATURES) == set(re.findall(r"\b(hicmi_[a-z0-9_]+)\(", text)) - {"hicmi_ctx"}


def test_the_store_form_is_read_at_every_call_and_the_constants_are_named():
    with open(os.path.join(CSRC, "api_pairs.inc")) as fh:
        api = fh.read()
    assert 'getenv("HICMI_PAIRS_PLAIN")' in api and api.count("pairs_plain()") == 3            # a definition and two uses
    assert 'getenv("HICMI_PAIRS_FIRST_PAIRS")' in api and api.count("pairs_first_setting(") == 2
    for path in (os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".inc"))):
        with open(path) as fh:
            assert not [ln for ln in fh if "HICMI_PAIRS_" in ln and re.search(r"\bstatic\b[^;]*\bgetenv\(", ln)], path
    with open(os.path.join(CSRC, "api.hip")) as fh:
        assert fh.read().count('#include "api_pairs.inc"') == 1
    with open(os.path.join(CSRC, "hicmi_internal.h")) as fh:
        internal = fh.read()
    for name in ("PAIRS_SLICE", "PAIRS_SLOT_BITS", "PAIRS_SLOTS", "PAIRS_PROBES"):
        assert re.search(r"static constexpr int %s = " % name, internal), name
    with open(os.path.join(CSRC, "k_pairs.hip")) as fh:
        kernel = fh.read()
    assert "static_assert((PAIRS_SLOTS & (PAIRS_SLOTS - 1)) == 0" in kernel and "static_assert(PAIRS_SLICE % 256 == 0" in kernel
    assert "k_pairs_keep<true>" in kernel and "k_pairs_keep<false>" in kernel and "__launch_bounds__(256)" in kernel
    with open(os.path.join(CSRC, "pairs.h")) as fh:
        head = fh.read()
    assert re.findall(r"#include\s+([<\"][^>\"]+[>\"])", head) == ['"anchor.h"']            # no GPU dependency
    assert re.search(r"constexpr int64_t PAIRS_FIRST_PAIRS = \(int64_t\)1 << 22;", head)
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    assert " pairs.h " in make and " k_pairs.hip " in make and "\napi.o: api_pairs.inc\n" in make
    # the store calls are not readers of the contact matrix, of a map build or of a span build, and the resident calls go
    # through the existing open / count / close path
    for word in ("c->dC", "map_cells", "drop_matrix_state", "span_marks", "span_grid", "map_m"):
        assert word not in api, word
    for word in ("ends_number(", "ends_open(", "launch_ends_count(", "ends_close(", "ends_plain()", "anchor_number(", "anchor_open(",
                 "launch_anchor_count(", "anchor_close(", "anchor_plain()", "pair_file_pass(", "check_pairs("):
        assert word in api, word
