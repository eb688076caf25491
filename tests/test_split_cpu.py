"""splitScaffolds without a GPU: tests/split_reference.py against its own brute-force spanning count,
csrc/split.h built as host code with the sanitizers and compared line by line with the reference, the cuts file and the
pieces, the writers, the native pair-file rewriter against a Python one, the declarations, and the command line on a fake
context that answers from the references.  Every comparison is exact."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import buildmap_reference as bref
import split_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")


# ---- the reference against itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_reference_spanning_equals_the_brute_force_count(seed):
    sizes, cuts, pairs = ref.random_case(seed)
    first, start, size, parent = ref.make_pieces(sizes, cuts)
    c = ref.counters(pairs, sizes, first, start)
    span = ref.spanning(first, c[3])
    assert span.tobytes() == ref.brute_spanning(pairs, sizes, first, start).tobytes()
    assert not span[first[1:] - 1].any()                                        # 0 at every parent's last piece
    # every pair counts once within, or once at each of two pieces
    assert int(c[0].sum()) + (int(c[1].sum()) + int(c[2].sum())) // 2 == len(pairs[0])
    ka, xa, kb, xb = ref.split_pairs(pairs, sizes, first, start)
    assert (parent[ka] == pairs[0]).all() and (xa >= 1).all() and (xa <= size[ka]).all() and (xa + start[ka] == pairs[1]).all()
    assert (parent[kb] == pairs[2]).all() and (xb >= 1).all() and (xb <= size[kb]).all() and (xb + start[kb] == pairs[3]).all()


def test_reference_on_a_hand_worked_case():
    sizes = np.array([10, 0, 7], np.int64)
    first, start, size, parent = ref.make_pieces(sizes, {0: [7, 3, 3], 2: [6]})
    assert first.tolist() == [0, 3, 4, 6] and start.tolist() == [0, 3, 7, 0, 0, 6] and size.tolist() == [3, 4, 3, 0, 6, 1]
    assert parent.tolist() == [0, 0, 0, 1, 2, 2]
    assert ref.piece_names(["a", "b", "c"], first) == ["a.brk1", "a.brk2", "a.brk3", "b", "c.brk1", "c.brk2"]
    pairs = (np.array([0, 0, 0, 0, 2]), np.array([3, 4, 1, 8, 7]), np.array([0, 0, 0, 2, 2]), np.array([1, 7, 10, 6, 7]))
    ka, xa, kb, xb = ref.split_pairs(pairs, sizes, first, start)
    assert ka.tolist() == [0, 1, 0, 2, 5] and xa.tolist() == [3, 1, 1, 1, 1]
    assert kb.tolist() == [0, 1, 2, 4, 5] and xb.tolist() == [1, 4, 3, 6, 1]
    c = ref.counters(pairs, sizes, first, start)
    assert c[0].tolist() == [1, 1, 0, 0, 0, 1] and c[1].tolist() == [1, 0, 1, 0, 0, 0] and c[2].tolist() == [0, 0, 1, 0, 1, 0]
    assert c[3].tolist() == [1, 0, 2 ** 64 - 1, 0, 0, 0] and ref.spanning(first, c[3]).tolist() == [1, 1, 0, 0, 0, 0]


# ---- split.h as host code under the sanitizers ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("split")
    exe = str(d / "split_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "split_host_check.cpp"), "-o", exe])

    def run(sizes, first, start, pairs):
        def row(a):
            return " ".join(str(int(x)) for x in a)
        lines = ["T %d %d" % (len(sizes), len(start)), row(sizes), row(first), row(start), "P %d" % len(pairs[0])]
        lines += ["%d %d %d %d" % r for r in zip(*(np.asarray(x).tolist() for x in pairs))]
        path = str(d / "case.txt")
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        # an ordinary child process, nothing preloaded
        done = subprocess.run([exe, path], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        return done.stdout.splitlines()
    return run


NO_PAIRS = (np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int64))


def _same_as_the_reference(got, sizes, first, start, pairs):
    ka, xa, kb, xb = ref.split_pairs(pairs, sizes, first, start)
    want = ["check 0 "] + ["pair %d %d %d %d" % r for r in zip(ka.tolist(), xa.tolist(), kb.tolist(), xb.tolist())]
    want += ["counter %d" % v for v in ref.counters(pairs, sizes, first, start).reshape(-1).tolist()]
    assert got == want                                                         # no "scan" line: both forms agree


@pytest.mark.parametrize("seed", range(8))
def test_native_pieces_and_counters_under_the_sanitizers(seed, host_check):
    sizes, cuts, pairs = ref.random_case(seed)
    first, start, _size, _parent = ref.make_pieces(sizes, cuts)
    _same_as_the_reference(host_check(sizes, first, start, pairs), sizes, first, start, pairs)


def piece_count_case(top=2 ** 33 + 70):
    """Scaffolds of 1, 2, 3, 64 and 65 pieces, one of one base, one without a base, and one above 2^32 bases cut above 2^32
    and into pieces of one base at either end."""
    sizes = np.array([50, 50, 1, 0, 50, 200, 200, top, 9], np.int64)
    cuts = {1: [25], 4: [1, 49], 5: list(range(3, 3 * 64, 3)), 6: list(range(2, 2 * 65, 2)),
            7: [1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33, top - 1], 8: [1, 8]}
    first, start, _size, _parent = ref.make_pieces(sizes, cuts)
    assert np.diff(first).tolist() == [1, 2, 1, 1, 3, 64, 65, 8, 3]
    return sizes, cuts, first, start


def test_native_every_cut_edge_and_piece_count_under_the_sanitizers(host_check):
    sizes, cuts, first, start = piece_count_case()
    ends = ref.edge_ends(sizes, cuts)
    assert (7, 2 ** 32 + 2) in ends and (7, int(sizes[7])) in ends and (4, 2) in ends and (2, 1) in ends
    rng = np.random.default_rng(5)
    pick = [ends[k] for k in rng.choice(len(ends), 60, replace=False)] + [e for e in ends if e[0] in (4, 7, 8)]
    pairs = ref.all_pairs(pick)
    _same_as_the_reference(host_check(sizes, first, start, pairs), sizes, first, start, pairs)
    # every edge end once, against itself
    pairs = ref.all_pairs(ends)[:2] * 2
    _same_as_the_reference(host_check(sizes, first, start, pairs), sizes, first, start, pairs)


def bad_tables():
    """(word of the message, sizes, piece_first, piece_start) for every refusal of split_check_tables."""
    sizes = [10, 0, 7]
    return [("piece 0", sizes, [1, 3, 4, 6], [0, 3, 7, 0, 0, 6]),
            ("scaffold 1 has the pieces", sizes, [0, 3, 3, 6], [0, 3, 7, 0, 0, 6]),
            ("scaffold 0 has the pieces", sizes, [0, 7, 4, 6], [0, 3, 7, 0, 0, 6]),
            ("scaffold 2 ends at piece 5", sizes, [0, 3, 4, 5], [0, 3, 7, 0, 0, 6]),
            ("scaffold 2 has the pieces", sizes, [0, 3, 4, 7], [0, 3, 7, 0, 0, 6]),
            ("first piece of scaffold 2", sizes, [0, 3, 4, 6], [0, 3, 7, 0, 1, 6]),
            ("piece 2 of scaffold 0", sizes, [0, 3, 4, 6], [0, 3, 3, 0, 0, 6]),          # not strictly ascending
            ("piece 2 of scaffold 0", sizes, [0, 3, 4, 6], [0, 8, 7, 0, 0, 6]),          # descending
            ("piece 1 of scaffold 0", sizes, [0, 3, 4, 6], [0, 10, 7, 0, 0, 6]),         # at the size
            ("piece 1 of scaffold 0", sizes, [0, 3, 4, 6], [0, 0, 7, 0, 0, 6]),          # a second start of 0
            ("piece 1 of scaffold 2", sizes, [0, 3, 4, 6], [0, 3, 7, 0, 0, 7]),          # at the size
            ("scaffold 1 has no base and 2 pieces", sizes, [0, 3, 5, 6], [0, 3, 7, 0, 0, 0]),
            ("negative size", [10, -1, 7], [0, 3, 4, 6], [0, 3, 7, 0, 0, 6])]


def test_native_table_refusals_under_the_sanitizers(host_check):
    for word, sizes, first, start in bad_tables():
        got = host_check(sizes, first, start, NO_PAIRS)
        assert len(got) == 1 and got[0].startswith("check -1 ") and word in got[0], (word, got)
    assert host_check([10, 0, 7], [0, 3, 4, 6], [0, 3, 7, 0, 0, 6], NO_PAIRS)[0] == "check 0 "


# ---- header, binding, switch -----------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_exports():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = re.sub(r"\s+", " ", fh.read())
    tables = "const int32_t *piece_first, const int64_t *piece_start, int64_t n_piece"
    assert ("int hicmi_split_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b, "
            "const int64_t *pos_b, int64_t n, const int64_t *scaf_size, int64_t n_scaf, " + tables + ", int32_t *piece_a_out, "
            "int64_t *pos_a_out, int32_t *piece_b_out, int64_t *pos_b_out, uint64_t *counters_out);") in text
    assert ("int hicmi_split_maps(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names, "
            "const int64_t *scaf_size, " + tables + ", int64_t n_res, const int64_t *resolution, hicmi_ctx *const *ctxs, "
            "int threads, int64_t *stats5, uint64_t *counters_out);") in text
    assert ("int hicmi_split_valid_pairs(const char *path_in, const char *path_out, const char *names_blob, "
            "const int64_t *name_off, int64_t n_names, const int64_t *scaf_size, " + tables + ", const char *piece_names_blob, "
            "const int64_t *piece_name_off, int threads, int64_t *stats4);") in text
    lib = _lib.load()
    for name, n_args in {"hicmi_split_pairs": 16, "hicmi_split_maps": 14, "hicmi_split_valid_pairs": 13}.items():
        assert len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
    assert callable(_lib.Context.split_pairs) and callable(_lib.split_maps) and callable(_lib.split_valid_pairs)
    assert lib.hicmi_abi_version() == 1
    assert set(_lib.SIGNATURES) == set(re.findall(r"\b(hicmi_[a-z0-9_]+)\(", text)) - {"hicmi_ctx"}


def test_the_kernel_form_is_read_at_every_call_and_the_constants_are_named():
    with open(os.path.join(CSRC, "api.hip")) as fh:
        api = fh.read()
    assert 'getenv("HICMI_SPLIT_PLAIN")' in api and api.count("split_plain()") == 3         # a definition and two uses
    for path in (os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))):
        with open(path) as fh:
            assert not [ln for ln in fh if "HICMI_SPLIT_PLAIN" in ln and re.search(r"\bstatic\b[^;]*\bgetenv\(", ln)], path
    with open(os.path.join(CSRC, "hicmi_internal.h")) as fh:
        internal = fh.read()
    for name in ("SPLIT_SLICE", "SPLIT_SLOTS", "SPLIT_PROBES", "SPLIT_MAX_BLOCKS"):
        assert re.search(r"static constexpr int %s = " % name, internal), name
    with open(os.path.join(CSRC, "split.h")) as fh:
        includes = re.findall(r"#include\s+([<\"][^>\"]+[>\"])", fh.read())
    assert includes == ['"liftmap.h"']                                                       # no GPU dependency
    with open(os.path.join(CSRC, "Makefile")) as fh:
        make = fh.read()
    assert " split.h " in make and " k_split.hip " in make
    # one chunk loop: the split pass is an argument of build_maps_loop, and the split calls read no contact matrix
    assert api.count("static int build_maps_loop(") == 1 and api.count("hicmi_parse_valid_pairs(") == 1
    with open(os.path.join(CSRC, "api_pairs.inc")) as fh:
        assert fh.read().count("hicmi_parse_valid_pairs(") == 0
    split_code = api[api.index("struct SplitHost"):api.index("// The chunk loop of hicmi_build_maps")]
    assert "c->dC" not in split_code and "map_cells" not in split_code and "drop_matrix_state" not in split_code


def test_spanning_of_the_binding_is_the_reference_prefix_sum():
    from hic_genome_assembler_amd import _lib
    for seed in range(4):
        sizes, cuts, pairs = ref.random_case(seed)
        first, start, _size, _parent = ref.make_pieces(sizes, cuts)
        c = ref.counters(pairs, sizes, first, start)
        assert _lib.split_spanning(first, c).tobytes() == ref.spanning(first, c[3]).tobytes()


# ---- the cuts file and the pieces ---------------------------------------------------------------------------------------------
NAMES = ["scaf_1", "scaf_2", "scaf_3", "scaf_4"]
SIZES = np.array([100, 40, 1, 60], np.int64)


def _write(path, text):
    with open(str(path), "w", newline="") as fh:
        fh.write(text)
    return str(path)


def test_parse_cuts_merges_repeats_and_skips_comments(tmp_path):
    from hic_genome_assembler_amd import splitScaffolds as ss
    path = _write(tmp_path / "cuts.tsv", "#scaffold\tcut_after\tratio\nscaf_1\t70\t0.01\n\nscaf_4\t5\nscaf_1\t30\t0.1\tmore\r\n"
                                         "scaf_1\t70\t0.02\n  \nscaf_1\t 31 \n")
    assert ss.parse_cuts(path) == {"scaf_1": [30, 31, 70], "scaf_4": [5]}
    # the cut files of two supportSpans runs, one after the other
    both = _write(tmp_path / "both.tsv", "scaf_1\t70\t0.01\nscaf_4\t5\t0.1\n" + "scaf_1\t70\t0.01\nscaf_1\t20\t0.05\n")
    assert ss.parse_cuts(both) == {"scaf_1": [20, 70], "scaf_4": [5]}
    for text, word in (("scaf_1\t7.5\n", "not an integer"), ("scaf_1\tx\n", "not an integer"), ("scaf_1\n", "no cut_after")):
        with pytest.raises(ValueError, match=word):
            ss.parse_cuts(_write(tmp_path / "bad.tsv", text))


def test_make_pieces_names_tables_and_min_piece():
    from hic_genome_assembler_amd import splitScaffolds as ss
    p = ss.make_pieces(NAMES, SIZES, {"scaf_1": [30, 31, 70], "scaf_4": [5]})
    assert p.names == ["scaf_1.brk1", "scaf_1.brk2", "scaf_1.brk3", "scaf_1.brk4", "scaf_2", "scaf_3", "scaf_4.brk1", "scaf_4.brk2"]
    first, start, size, parent = ref.make_pieces(SIZES, {0: [30, 31, 70], 3: [5]})
    assert p.piece_first.dtype == np.int32 and p.piece_start.dtype == np.int64
    assert p.piece_first.tolist() == first.tolist() and p.piece_start.tolist() == start.tolist()
    assert p.sizes.tolist() == size.tolist() and p.parent.tolist() == parent.tolist() and p.names == ref.piece_names(NAMES, first)
    assert p.applied == {"scaf_1": [30, 31, 70], "scaf_4": [5]} and p.skipped == []
    # -minPiece 10: 31 lies 1 base after the kept 30, 5 lies 5 bases after the left end; 95 lies 5 before the right end
    p = ss.make_pieces(NAMES, SIZES, {"scaf_1": [30, 31, 70, 95], "scaf_4": [5], "scaf_2": [10, 30]}, 10)
    assert p.applied == {"scaf_1": [30, 70], "scaf_2": [10, 30]} and p.skipped == [("scaf_1", 31), ("scaf_1", 95), ("scaf_4", 5)]
    assert p.names == ["scaf_1.brk1", "scaf_1.brk2", "scaf_1.brk3", "scaf_2.brk1", "scaf_2.brk2", "scaf_2.brk3", "scaf_3", "scaf_4"]
    # a skipped cut does not shield the next one: 25 is skipped (5 after 20), 30 is kept (10 after 20)
    assert ss.make_pieces(NAMES, SIZES, {"scaf_1": [20, 25, 30]}, 10).applied == {"scaf_1": [20, 30]}
    for cuts, word in (({"zz": [5]}, "zz"), ({"scaf_1": [0]}, "outside 1"), ({"scaf_1": [100]}, "outside 1"), ({"scaf_3": [1]}, "outside 1"),
                       ({"scaf_2": [-4]}, "outside 1")):
        with pytest.raises(ValueError, match=word):
            ss.make_pieces(NAMES, SIZES, cuts)
    with pytest.raises(ValueError, match="minPiece"):
        ss.make_pieces(NAMES, SIZES, {}, 0)
    with pytest.raises(ValueError, match="scaf_1.brk2 is already"):
        ss.make_pieces(NAMES + ["scaf_1.brk2"], np.append(SIZES, 5), {"scaf_1": [50]})
    # a name of that shape is no clash while its parent stays whole
    assert ss.make_pieces(NAMES + ["scaf_1.brk2"], np.append(SIZES, 5), {"scaf_2": [5]}).names[0] == "scaf_1"


# ---- the writers ------------------------------------------------------------------------------------------------------------
def _pieces():
    from hic_genome_assembler_amd import splitScaffolds as ss
    return ss, ss.make_pieces(NAMES, SIZES, {"scaf_1": [30, 70], "scaf_4": [5]})


def test_sizes_and_agp():
    ss, p = _pieces()
    assert ss.sizes_text(p) == "scaf_1.brk1\t30\nscaf_1.brk2\t40\nscaf_1.brk3\t30\nscaf_2\t40\nscaf_3\t1\nscaf_4.brk1\t5\nscaf_4.brk2\t55\n"
    assert ss.agp_text(p, NAMES).splitlines() == [
        "##agp-version\t2.0", "scaf_1.brk1\t1\t30\t1\tW\tscaf_1\t1\t30\t+", "scaf_1.brk2\t1\t40\t1\tW\tscaf_1\t31\t70\t+",
        "scaf_1.brk3\t1\t30\t1\tW\tscaf_1\t71\t100\t+", "scaf_2\t1\t40\t1\tW\tscaf_2\t1\t40\t+", "scaf_3\t1\t1\t1\tW\tscaf_3\t1\t1\t+",
        "scaf_4.brk1\t1\t5\t1\tW\tscaf_4\t1\t5\t+", "scaf_4.brk2\t1\t55\t1\tW\tscaf_4\t6\t60\t+"]


def test_fasta_pieces_concatenate_to_the_parent(tmp_path):
    from hic_genome_assembler_amd.writeAssembledFasta import readFastaIntoMem
    ss, p = _pieces()
    rng = np.random.default_rng(3)
    fasta = {name: "".join(rng.choice(list("ACGTNacgt"), int(L))) for name, L in zip(NAMES, SIZES)}
    fasta = dict([("extra_contig", "ACGT" * 30)] + list(fasta.items()))              # an entry the size file does not have
    ss.check_fasta(fasta, p, NAMES, SIZES)
    out = str(tmp_path / "split.fasta")
    ss.write_fasta(out, fasta, p, NAMES)
    got = readFastaIntoMem(out)
    assert list(got) == ["extra_contig"] + p.names and got["extra_contig"] == fasta["extra_contig"]
    for s, name in enumerate(NAMES):
        parts = [got[p.names[k]] for k in range(p.piece_first[s], p.piece_first[s + 1])]
        assert "".join(parts) == fasta[name] and [len(x) for x in parts] == p.sizes[p.piece_first[s]:p.piece_first[s + 1]].tolist()
    with open(out) as fh:
        lines = fh.read().splitlines()
    assert max(len(ln) for ln in lines) == 50 and lines[lines.index(">scaf_1.brk2") + 1] == fasta["scaf_1"][30:70]
    with pytest.raises(ValueError, match="99 bases"):
        ss.check_fasta(dict(fasta, scaf_1=fasta["scaf_1"][:99]), p, NAMES, SIZES)
    with pytest.raises(ValueError, match="scaf_4 is cut"):
        ss.check_fasta({k: v for k, v in fasta.items() if k != "scaf_4"}, p, NAMES, SIZES)


def test_restriction_sites_at_the_cut_edges():
    ss, p = _pieces()
    lines = ["scaf_1\t0\t0\tHIC_scaf_1_1\t0\t+\n", "scaf_1\t0\t30\tf2\n", "scaf_1\t30\t31\tf3\r\n", "scaf_1\t25\t70\tf4\n",
             "scaf_1\t70\t71\n", "scaf_1\t71\t100\tf6\n", "scaf_2\t0\t40\tf7\n", "other\tx\ty\n", "scaf_4\t3\t6\tf8"]
    assert ss.restriction_text(lines, p, NAMES).splitlines(keepends=True) == [
        "scaf_1.brk1\t0\t0\tHIC_scaf_1_1\t0\t+\n", "scaf_1.brk1\t0\t30\tf2\n", "scaf_1.brk2\t0\t1\tf3\r\n", "scaf_1.brk2\t0\t40\tf4\n",
        "scaf_1.brk3\t0\t1\n", "scaf_1.brk3\t1\t30\tf6\n", "scaf_2\t0\t40\tf7\n", "other\tx\ty\n", "scaf_4.brk2\t0\t1\tf8"]
    with pytest.raises(ValueError, match="line 2"):
        ss.restriction_text(["scaf_2\t1\t2\n", "scaf_1\t1\n"], p, NAMES)


def test_order_file_for_plus_and_minus_parents():
    ss, p = _pieces()
    lines = ["### Chromosome grouping 1 ###\n", "scaf_2\t-\n", "scaf_1\t-\n", "scaf_3\t+\textra\n", "### Chromosome grouping 2 ###\r\n",
             "scaf_4\t+\r\n", "unknown\t?"]
    assert ss.order_text(lines, p).splitlines(keepends=True) == [
        "### Chromosome grouping 1 ###\n", "scaf_2\t-\n", "scaf_1.brk3\t-\n", "scaf_1.brk2\t-\n", "scaf_1.brk1\t-\n", "scaf_3\t+\textra\n",
        "### Chromosome grouping 2 ###\r\n", "scaf_4.brk1\t+\r\n", "scaf_4.brk2\t+\r\n", "unknown\t?"]
    with pytest.raises(ValueError, match="line 2"):
        ss.order_text(["### 1 ###\n", "scaf_1\t?\n"], p)


# ---- the native rewriter of the pair file -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def odd_case(tmp_path_factory):
    """The 40 odd scaffolds of the buildMap tests, eight of them cut, and a 3000-line file with CRLF lines, 6 and 12 columns,
    skipped lines of both kinds and no final newline."""
    names, sizes = bref.odd_scaffolds()
    cuts = {3: [1000, 1001, 35000, 69999], 17: [1], 38: [500, 64000], 4: [1000, 3000], 9: [1], 14: [3006], 0 + 2: [999], 13: [500]}
    first, start, size, _parent = ref.make_pieces(sizes, cuts)
    data = bref.odd_file_bytes(names, sizes, 3000, 77)
    assert b"\r\n" in data and not data.endswith(b"\n")
    path = str(tmp_path_factory.mktemp("pairs") / "odd.allValidPairs")
    with open(path, "wb") as fh:
        fh.write(data)
    return {"names": names, "sizes": sizes, "first": first, "start": start, "piece_sizes": size, "piece_names": ref.piece_names(names, first),
            "data": data, "path": path}


def _rewrite(case, out, threads, path=None):
    from hic_genome_assembler_amd import _lib
    return _lib.split_valid_pairs(path or case["path"], out, case["names"], case["sizes"], case["first"], case["start"],
                                  case["piece_names"], threads=threads)


def test_native_rewriter_equals_the_python_rewriter_at_every_thread_count(odd_case, tmp_path):
    want, stats = ref.rewrite_pair_file(odd_case["data"], odd_case["names"], odd_case["sizes"], odd_case["first"], odd_case["start"],
                                        odd_case["piece_names"])
    assert stats[2] > 50 and stats[3] > 50 and stats[1] > 2000 and b"\r\n" in want and b".brk" in want
    assert stats == bref.parse_text(odd_case["data"], odd_case["names"], odd_case["sizes"])[1]
    for threads in (1, 3, 16):
        out = str(tmp_path / ("out%d" % threads))
        assert _rewrite(odd_case, out, threads) == stats
        with open(out, "rb") as fh:
            assert fh.read() == want
        assert os.listdir(str(tmp_path)) == ["out%d" % threads]                          # no temporary file stays
        os.remove(out)


def test_rewritten_file_parses_to_the_reference_split_pairs(odd_case, tmp_path):
    from hic_genome_assembler_amd import _lib
    out = str(tmp_path / "split.allValidPairs")
    _rewrite(odd_case, out, 3)
    pairs, stats, _after = bref.parse_text(odd_case["data"], odd_case["names"], odd_case["sizes"])
    want = ref.split_pairs(pairs, odd_case["sizes"], odd_case["first"], odd_case["start"])
    sa, pa, sb, pb, _next, got_stats = _lib.parse_valid_pairs(out, odd_case["piece_names"], odd_case["piece_sizes"])
    assert got_stats == (stats[1], stats[1], 0, 0)
    for got, exp in zip((sa, pa, sb, pb), want):
        assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes()


def test_a_malformed_line_is_the_parsers_error_and_leaves_no_output(odd_case, tmp_path):
    from hic_genome_assembler_amd import _lib
    lines = odd_case["data"].split(b"\n")
    for where, bad in ((0, b"r\tscaffold_1\t5\t+\tscaffold_2"), (1500, b"r\tscaffold_1\t5x\t+\tscaffold_2\t1\t-"), (2999, b"r\tscaffold_1\t5\t+\tscaffold_2\t\t-")):
        broken = lines[:where] + [bad] + lines[where + 1:]
        path = str(tmp_path / "broken.allValidPairs")
        with open(path, "wb") as fh:
            fh.write(b"\n".join(broken))
        offset = len(b"\n".join(broken[:where])) + (1 if where else 0)
        with pytest.raises(bref.Malformed) as exc:
            bref.parse_text(b"\n".join(broken), odd_case["names"], odd_case["sizes"])
        assert exc.value.offset == offset
        for threads in (1, 16):
            with pytest.raises(_lib.HicmiError, match="malformed valid-pair line at byte %d$" % offset):
                _rewrite(odd_case, str(tmp_path / "out"), threads, path=path)
            assert sorted(os.listdir(str(tmp_path))) == ["broken.allValidPairs"]
    # bad tables and a missing input are refused in the same way
    with pytest.raises(_lib.HicmiError, match="first piece of scaffold 0"):
        _lib.split_valid_pairs(odd_case["path"], str(tmp_path / "out"), odd_case["names"], odd_case["sizes"], odd_case["first"],
                               odd_case["start"] + 1, odd_case["piece_names"])
    with pytest.raises(_lib.HicmiError, match="cannot open"):
        _rewrite(odd_case, str(tmp_path / "out"), 1, path=str(tmp_path / "nothing_here"))
    assert sorted(os.listdir(str(tmp_path))) == ["broken.allValidPairs"]


# ---- the command line on a fake context --------------------------------------------------------------------------------------------
class FakeMap:
    def __init__(self, dense):
        self.dense, self.closed = dense, False

    def contacts_host(self):
        return self.dense.copy()

    def close(self):
        self.closed = True


class FakeDevice:
    """The two device calls of splitScaffolds.runPipeline, answered by the references (and by the library's host code)."""

    def __init__(self):
        self.calls, self.maps = [], []

    def split_maps(self, path, names, sizes, piece_first, piece_start, resolutions, threads):
        with open(path, "rb") as fh:
            pairs, stats, _after = bref.parse_text(fh.read(), names, sizes)
        moved = ref.split_pairs(pairs, sizes, piece_first, piece_start)
        last = np.zeros(len(piece_start), bool)
        last[np.asarray(piece_first[1:]) - 1] = True
        parent = np.repeat(np.arange(len(sizes)), np.diff(piece_first))
        piece_sizes = np.where(last, np.asarray(sizes)[parent], np.append(piece_start[1:], 0)) - piece_start
        self.maps = [FakeMap(bref.build(moved, piece_sizes, r)) for r in resolutions]
        self.calls.append(("split_maps", tuple(resolutions)))
        return stats + (1,), ref.counters(pairs, sizes, piece_first, piece_start), self.maps

    def split_valid_pairs(self, path_in, path_out, names, sizes, piece_first, piece_start, piece_names, threads):
        from hic_genome_assembler_amd import _lib
        self.calls.append(("split_valid_pairs", os.path.basename(path_out)))
        return _lib.split_valid_pairs(path_in, path_out, names, sizes, piece_first, piece_start, piece_names, threads=threads)


CLI_NAMES = ["chr1_a", "chr1_b", "tiny", "chr2_a", "chr2_b"]
CLI_SIZES = np.array([9000, 4000, 1, 7000, 2500], np.int64)
CLI_CUTS = {"chr1_a": [3000, 3010, 6000], "chr2_a": [6975]}


def _cli_files(tmp_path, pair_file=True, order=True, fasta=True, sites=True):
    from hic_genome_assembler_amd import synth
    d = str(tmp_path)
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    _write(paths["hicProScaffSizeFile"], "".join("%s\t%d\n" % ns for ns in zip(CLI_NAMES, CLI_SIZES.tolist())))
    save = os.path.join(d, "save")
    extra = {}
    rng = np.random.default_rng(2)
    n = 1500
    sa, sb = rng.integers(0, 5, n), rng.integers(0, 5, n)
    cis = rng.random(n) < 0.7
    sb[cis] = sa[cis]
    pa = 1 + np.floor(rng.random(n) * CLI_SIZES[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * CLI_SIZES[sb]).astype(np.int64)
    pairs = (sa.astype(np.int32), pa, sb.astype(np.int32), pb)
    if pair_file:
        extra["validPairFile"] = os.path.join(d, "in.allValidPairs")
        text = "".join("r%d\t%s\t%d\t+\t%s\t%d\t-\t300\tfrag_%d\tfrag_%d\t42\t42\n" % (k, CLI_NAMES[a], x, CLI_NAMES[b], y, k, k + 1)
                       for k, (a, x, b, y) in enumerate(zip(*(v.tolist() for v in pairs))))
        text += "r\tnot_there\t5\t+\tchr1_a\t5\t-\nr\tchr1_a\t9001\t+\tchr1_a\t5\t-\n"
        _write(extra["validPairFile"], text)
    if fasta:
        extra["originalFastaFile"] = os.path.join(d, "genome.fasta")
        _write(extra["originalFastaFile"], "".join(">%s\n%s\n" % (nm, "".join(rng.choice(list("ACGT"), int(L)))) for nm, L in zip(CLI_NAMES, CLI_SIZES)))
    if sites:
        extra["restrictionSiteFile"] = os.path.join(d, "sites.bed")
        _write(extra["restrictionSiteFile"], "".join("%s\t%d\t%d\tHIC_%s_%d\t0\t+\n" % (nm, a, a + 500, nm, k)
                                                        for nm, L in zip(CLI_NAMES, CLI_SIZES) for k, a in enumerate(range(0, int(L), 500))))
    cfg = synth.write_config(os.path.join(d, "config.txt"), paths, save, os.path.join(d, "plots"), 100000, extra=extra)
    if order:
        _write(os.path.join(save, "chromosomeOrders.txt"), "### Chromosome grouping 1 ###\nchr1_b\t+\nchr1_a\t-\n### Chromosome grouping 2 ###\n"
                                                           "chr2_a\t+\nchr2_b\t-\n")
    cuts = _write(os.path.join(d, "cuts.tsv"), "".join("%s\t%d\t0.01\n" % (nm, c) for nm, cs in CLI_CUTS.items() for c in cs))
    return cfg, cuts, save, pairs


def _config_values(path):
    with open(path) as fh:
        return dict(ln.rstrip("\n").split(" = ", 1) for ln in fh if " = " in ln and not ln.startswith("#"))


def test_cli_on_a_fake_context(tmp_path, capsys):
    from hic_genome_assembler_amd import splitScaffolds as ss
    cfg, cuts, save, pairs = _cli_files(tmp_path)
    fake = FakeDevice()
    ss.main(["-config", cfg, "-cuts", cuts, "-resolution", "1000,2500", "-minPiece", "20", "-noBalance", "-threads", "2"], context=fake)
    out = os.path.join(save, "split")
    assert fake.calls == [("split_maps", (1000, 2500)), ("split_valid_pairs", "split.allValidPairs")] and all(m.closed for m in fake.maps)
    assert sorted(os.listdir(out)) == ["chromosomeOrders.txt", "res1000", "res2500", "split.agp", "split.allValidPairs", "split.fasta",
                                       "split.restriction.bed", "split.sizes", "split_summary.tsv"]
    first, start, size, parent = ref.make_pieces(CLI_SIZES, {0: [3000, 6000], 3: [6975]})
    new_names = ref.piece_names(CLI_NAMES, first)
    with open(os.path.join(out, "split.sizes")) as fh:
        assert fh.read() == "".join("%s\t%d\n" % ns for ns in zip(new_names, size.tolist()))
    with open(os.path.join(out, "chromosomeOrders.txt")) as fh:
        assert fh.read() == ("### Chromosome grouping 1 ###\nchr1_b\t+\nchr1_a.brk3\t-\nchr1_a.brk2\t-\nchr1_a.brk1\t-\n"
                             "### Chromosome grouping 2 ###\nchr2_a.brk1\t+\nchr2_a.brk2\t+\nchr2_b\t-\n")
    with open(os.path.join(out, "split.restriction.bed")) as fh:
        sites = fh.read().splitlines()
    assert "chr1_a.brk1\t2500\t3000\tHIC_chr1_a_5\t0\t+" in sites and "chr1_a.brk2\t0\t500\tHIC_chr1_a_6\t0\t+" in sites
    assert "chr2_a.brk1\t6000\t6500\tHIC_chr2_a_12\t0\t+" in sites and "chr2_a.brk2\t0\t25\tHIC_chr2_a_13\t0\t+" in sites
    # the pair file: the fragment columns stay, the skipped lines are gone
    with open(os.path.join(tmp_path, "in.allValidPairs"), "rb") as fh:
        want, stats = ref.rewrite_pair_file(fh.read(), CLI_NAMES, CLI_SIZES, first, start, new_names)
    with open(os.path.join(out, "split.allValidPairs"), "rb") as fh:
        got = fh.read()
    assert got == want and stats == (1502, 1500, 1, 1) and b"\tfrag_7\tfrag_8\t" in got
    # the maps and the configs
    moved = ref.split_pairs(pairs, CLI_SIZES, first, start)
    for r in (1000, 2500):
        d = os.path.join(out, "res%d" % r)
        assert sorted(os.listdir(d)) == ["config.txt", "out", "plots", "split_%d.matrix" % r, "split_%d_abs.bed" % r]
        with open(os.path.join(d, "split_%d_abs.bed" % r)) as fh:
            assert [tuple(ln.split("\t")) for ln in fh.read().splitlines()] == [(n, str(a), str(b), str(i)) for n, a, b, i in bref.bed_rows(new_names, size, r)]
        dense = bref.build(moved, size, r)
        with open(os.path.join(d, "split_%d.matrix" % r)) as fh:
            cells = {(int(a), int(b)): float(x) for a, b, x in (ln.split("\t") for ln in fh.read().splitlines())}
        iu, ju = np.nonzero(np.triu(dense))
        assert cells == {(int(i) + 1, int(j) + 1): float(dense[i, j]) for i, j in zip(iu, ju)}
        val = _config_values(os.path.join(d, "config.txt"))
        assert val["resolution"] == str(r) and val["hicProBedFile"] == os.path.join(d, "split_%d_abs.bed" % r)
        assert val["hicProRawMatrixFile"] == os.path.join(d, "split_%d.matrix" % r) and val["hicProMatrixFile"] == os.path.join(d, "split_%d_iced.matrix" % r)
        assert val["hicProBiasFile"] == val["hicProMatrixFile"] + ".biases"
        assert val["saveFilesDirectory"] == os.path.join(d, "out") and val["savePlotsDirectory"] == os.path.join(d, "plots")
        assert val["hicProScaffSizeFile"] == os.path.join(out, "split.sizes") and val["validPairFile"] == os.path.join(out, "split.allValidPairs")
        assert val["restrictionSiteFile"] == os.path.join(out, "split.restriction.bed") and val["originalFastaFile"] == os.path.join(out, "split.fasta")
        assert val["chromosomeOrderFile"] == "chromosomeOrders.txt" and val["minSize"] == "5"
    # the summary
    c = ref.counters(pairs, CLI_SIZES, first, start)
    span = ref.brute_spanning(pairs, CLI_SIZES, first, start)
    with open(os.path.join(out, "split_summary.tsv")) as fh:
        lines = fh.read().splitlines()
    assert lines[0] == "#lines=1502\tused=1500\tunknown_scaffold=1\tout_of_range=1\tcuts=3\tskipped_cuts=1"
    assert lines[1] == "#skipped_cut\tchr1_a\t3010" and lines[2].startswith("#resolution\tbins\t") and lines[3].split("\t")[:2] == ["1000", "25"]
    assert lines[4].split("\t")[:4] == ["2500", "14", "8", "3"] and lines[5] == "#piece\tparent\tfirst_base\tlast_base\tsize\twithin\tsibling\tother\tspanning"
    last = set((first[1:] - 1).tolist())
    assert lines[6:] == ["\t".join([new_names[k], CLI_NAMES[parent[k]], str(start[k] + 1), str(start[k] + size[k]), str(size[k]), str(c[0, k]),
                                    str(c[1, k]), str(c[2, k]), "NA" if k in last else str(span[k])]) for k in range(len(size))]
    assert span[0] > 0 and span[1] > 0 and span[5] > 0 and len(lines) == 6 + 8
    assert "SPLIT: 3 cut(s) applied to 2 scaffold(s), 1 skipped, 8 piece(s)" in capsys.readouterr().out


def test_cli_without_pairs_resolutions_and_optional_files(tmp_path):
    from hic_genome_assembler_amd import splitScaffolds as ss
    cfg, cuts, save, _pairs = _cli_files(tmp_path, pair_file=False, order=False, fasta=False, sites=False)
    fake = FakeDevice()
    out = str(tmp_path / "elsewhere")
    ss.main(["-config", cfg, "-cuts", cuts, "-noPairs", "-out", out], context=fake)
    assert fake.calls == [] and sorted(os.listdir(out)) == ["split.agp", "split.sizes", "split_summary.tsv"]
    with open(os.path.join(out, "split_summary.tsv")) as fh:
        lines = fh.read().splitlines()
    assert lines[0] == "#lines=NA\tused=NA\tunknown_scaffold=NA\tout_of_range=NA\tcuts=4\tskipped_cuts=0"
    assert lines[3] == "chr1_a.brk1\tchr1_a\t1\t3000\t3000\tNA\tNA\tNA\tNA" and len(lines) == 3 + 9
    # with a pair file, -noPairs and no resolution still count the pieces
    os.mkdir(str(tmp_path / "b"))
    cfg, cuts, save, pairs = _cli_files(tmp_path / "b", order=False)
    ss.main(["-config", cfg, "-cuts", cuts, "-noPairs"], context=fake)
    assert fake.calls == [("split_maps", ())]
    assert sorted(os.listdir(os.path.join(save, "split"))) == ["split.agp", "split.fasta", "split.restriction.bed", "split.sizes", "split_summary.tsv"]


def test_bad_input_is_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import splitScaffolds as ss, synth
    cfg, cuts, save, _pairs = _cli_files(tmp_path, order=False)
    d = str(tmp_path)
    fake = FakeDevice()

    def refused(word, more=(), config=cfg, cuts_file=cuts):
        with pytest.raises(SystemExit) as exc:
            ss.main(["-config", config, "-cuts", cuts_file, "-resolution", "1000"] + list(more), context=fake)
        assert word in str(exc.value.code) and str(exc.value.code).startswith("ERROR... ") and \
            str(exc.value.code).endswith(" Exiting..."), exc.value.code

    refused("zz", cuts_file=_write(tmp_path / "c1", "zz\t5\n"))
    refused("not an integer", cuts_file=_write(tmp_path / "c2", "chr1_a\t5.5\n"))
    refused("outside 1", cuts_file=_write(tmp_path / "c3", "chr1_a\t0\n"))
    refused("outside 1", cuts_file=_write(tmp_path / "c4", "chr1_a\t9000\n"))
    refused("does not exist", cuts_file=os.path.join(d, "nothing_here"))
    refused("minPiece", ["-minPiece", "0"])
    refused("given twice", ["-resolution", "1000,1000"])
    refused("does not exist", ["-order", os.path.join(d, "nothing_here")])
    refused("orientation", ["-order", _write(tmp_path / "o1", "### 1 ###\nchr1_a\t?\n")])
    # more than 65,536 bins (22,501 bases and 65,537 bins of 1 bp more): what buildMap refuses
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile")}
    paths["hicProScaffSizeFile"] = _write(tmp_path / "long.sizes", "".join("%s\t%d\n" % ns for ns in zip(CLI_NAMES, CLI_SIZES.tolist()))
                                          + "long\t%d\n" % (65537 - 22501))
    long_cfg = synth.write_config(os.path.join(d, "long.txt"), paths, save, os.path.join(d, "plots"), 100000,
                                  extra={"validPairFile": os.path.join(d, "in.allValidPairs")})
    refused("resolution 1 needs 65537 bins, more than the 65536", ["-resolution", "1"], config=long_cfg)
    # a piece name the size file has already
    paths["hicProScaffSizeFile"] = _write(tmp_path / "clash.sizes", "chr1_a\t9000\nchr1_a.brk1\t5\n")
    clash = synth.write_config(os.path.join(d, "clash.txt"), paths, save, os.path.join(d, "plots"), 100000,
                               extra={"validPairFile": os.path.join(d, "in.allValidPairs")})
    refused("already a scaffold", config=clash, cuts_file=_write(tmp_path / "c5", "chr1_a\t50\n"))
    # no pair file: refused with a resolution, and without -noPairs
    paths["hicProScaffSizeFile"] = os.path.join(d, "hicProScaffSizeFile.txt")
    bare = synth.write_config(os.path.join(d, "bare.txt"), paths, save, os.path.join(d, "plots"), 100000)
    refused("validPairFile", config=bare)
    refused("validPairFile", ["-noPairs"], config=bare)
    with pytest.raises(SystemExit) as exc:
        ss.main(["-config", bare, "-cuts", cuts], context=fake)
    assert "validPairFile" in str(exc.value.code)
    # a FASTA that does not fit the size file
    short = synth.write_config(os.path.join(d, "short.txt"), paths, save, os.path.join(d, "plots"), 100000,
                               extra={"validPairFile": os.path.join(d, "in.allValidPairs"),
                                      "originalFastaFile": _write(tmp_path / "short.fasta", ">chr1_a\nACGT\n>chr2_a\nACGT\n")})
    refused("4 bases", config=short)
    assert fake.calls == [] and os.listdir(save) == []


def test_a_malformed_pair_line_ends_the_run_with_nothing_written(tmp_path):
    from hic_genome_assembler_amd import _lib, splitScaffolds as ss
    cfg, cuts, save, _pairs = _cli_files(tmp_path, order=False)
    with open(os.path.join(str(tmp_path), "in.allValidPairs"), "a") as fh:
        fh.write("r\tchr1_a\tfive\t+\tchr1_a\t5\t-\n")

    class Refusing(FakeDevice):
        def split_maps(self, path, *rest):
            try:
                return FakeDevice.split_maps(self, path, *rest)
            except bref.Malformed as exc:
                raise _lib.HicmiError("libhicmi error 2: %s" % exc)

    with pytest.raises(SystemExit) as exc:
        ss.main(["-config", cfg, "-cuts", cuts, "-resolution", "1000", "-noBalance"], context=Refusing())
    assert "malformed valid-pair line at byte" in str(exc.value.code) and os.listdir(save) == []
