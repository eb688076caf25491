"""assembledMap without a GPU: the layout builder and the lift against hand-worked cases and
tests/liftmap_reference.py, the AGP and size texts, the refusals of the command line, the decay slot, the declarations,
and the native lift / key / table-check code built as host code with the sanitizers.  Every comparison is exact."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import liftmap_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")

# five scaffolds a .. e; Chr_1 = c-, b-, a+ (b has one base), Chr_2 = d+ alone, e is not placed
NAMES = ["a", "b", "c", "d", "e"]
SIZES = np.array([5, 1, 7, 3, 4], dtype=np.int64)
GROUPS = [[["c", "-"], ["b", "-"], ["a", "+"]], [["d", "+"]]]
CHROMS = [[(2, "-"), (1, "-"), (0, "+")], [(3, "+")]]
# gap -> (offsets of c, b, a; size of Chr_1), worked by hand
HAND = {0: ((0, 7, 8), 13), 1: ((0, 8, 10), 15), 100: ((0, 107, 208), 213)}


@pytest.mark.parametrize("gap", sorted(HAND))
def test_layout_against_hand_worked_cases(gap):
    from hic_genome_assembler_amd import assembledMap as am
    (off_c, off_b, off_a), chr1 = HAND[gap]
    asm = am.build_assembly(GROUPS, NAMES, SIZES, gap)
    assert asm.seq_names == ["Chr_1", "Chr_2", "e"] and asm.seq_sizes.tolist() == [chr1, 3, 4] and asm.n_chromosomes == 2
    assert asm.lift_seq.tolist() == [0, 0, 0, 1, 2] and asm.lift_rev.tolist() == [0, 1, 1, 0, 0]
    assert asm.lift_off.tolist() == [off_a, off_b, off_c, 0, 0]
    assert asm.lift_seq.dtype == np.int32 and asm.lift_off.dtype == np.int64 and asm.lift_rev.dtype == np.uint8
    # the sequence's size is sum L + gap (S - 1); the one-scaffold chromosome has no gap
    assert chr1 == 5 + 1 + 7 + 2 * gap
    # positions 1 and L of a - scaffold land at off + L and off + 1; a size-1 scaffold reversed stays at off + 1
    seq, pos = am.lift(asm, SIZES, [2, 2, 1, 0, 0, 3, 4], [1, 7, 1, 1, 5, 2, 4])
    assert seq.tolist() == [0, 0, 0, 0, 0, 1, 2]
    assert pos.tolist() == [off_c + 7, off_c + 1, off_b + 1, off_a + 1, off_a + 5, 2, 4]
    # the reference's layout is the same tables
    tables = ref.layout(CHROMS, SIZES, gap)
    for got, want in zip((asm.lift_seq, asm.lift_off, asm.lift_rev, asm.seq_sizes), tables):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    for s in range(5):
        for p in range(1, int(SIZES[s]) + 1):
            q, x = am.lift(asm, SIZES, [s], [p])
            assert (int(q[0]), int(x[0])) == ref.lift_one(tables, SIZES, s, p)
    # dropped instead of appended
    only = am.build_assembly(GROUPS, NAMES, SIZES, gap, chromosomes_only=True)
    assert only.seq_names == ["Chr_1", "Chr_2"] and only.lift_seq.tolist() == [0, 0, 0, 1, -1]
    assert [x.tolist() for x in am.lift(only, SIZES, [4], [2])] == [[-1], [0]]
    assert [a.tobytes() for a in ref.layout(CHROMS, SIZES, gap, drop_unplaced=True)] == \
        [a.tobytes() for a in (only.lift_seq, only.lift_off, only.lift_rev, only.seq_sizes)]


def test_lifting_a_reversed_scaffold_twice_is_the_identity():
    from hic_genome_assembler_amd import assembledMap as am
    sizes = np.array([1, 2, 999, 2 ** 33], dtype=np.int64)
    names = ["s%d" % k for k in range(4)]
    asm = am.build_assembly([[[n, "-"]] for n in names], names, sizes, 100)
    assert asm.lift_off.tolist() == [0, 0, 0, 0] and asm.seq_sizes.tolist() == sizes.tolist()
    for s, L in enumerate(sizes.tolist()):
        p = np.unique(np.array([1, 2, L // 2 + 1, L - 1, L]).clip(1, L))
        _seq, once = am.lift(asm, sizes, np.full(len(p), s), p)
        assert once.tolist() == (L - p + 1).tolist()
        _seq, twice = am.lift(asm, sizes, np.full(len(p), s), once)
        assert twice.tolist() == p.tolist()


def test_agp_and_sizes_text():
    from hic_genome_assembler_amd import assembledMap as am
    asm = am.build_assembly(GROUPS, NAMES, SIZES, 100)
    assert am.sizes_text(asm) == "Chr_1\t213\nChr_2\t3\ne\t4\n"
    assert am.agp_text(asm, NAMES, SIZES) == (
        "##agp-version\t2.0\n"
        "Chr_1\t1\t7\t1\tW\tc\t1\t7\t-\n"
        "Chr_1\t8\t107\t2\tN\t100\tscaffold\tyes\tproximity_ligation\n"
        "Chr_1\t108\t108\t3\tW\tb\t1\t1\t-\n"
        "Chr_1\t109\t208\t4\tN\t100\tscaffold\tyes\tproximity_ligation\n"
        "Chr_1\t209\t213\t5\tW\ta\t1\t5\t+\n"
        "Chr_2\t1\t3\t1\tW\td\t1\t3\t+\n"
        "e\t1\t4\t1\tW\te\t1\t4\t+\n")
    # a gap of 0 gives no N line, and -chromosomesOnly no object for e
    none = am.build_assembly(GROUPS, NAMES, SIZES, 0, chromosomes_only=True)
    assert am.agp_text(none, NAMES, SIZES) == (
        "##agp-version\t2.0\n"
        "Chr_1\t1\t7\t1\tW\tc\t1\t7\t-\n"
        "Chr_1\t8\t8\t2\tW\tb\t1\t1\t-\n"
        "Chr_1\t9\t13\t3\tW\ta\t1\t5\t+\n"
        "Chr_2\t1\t3\t1\tW\td\t1\t3\t+\n")
    assert am.sizes_text(none) == "Chr_1\t13\nChr_2\t3\n"


def test_order_file_is_read_as_part_4_reads_it(tmp_path):
    from hic_genome_assembler_amd import assembledMap as am
    path = str(tmp_path / "orders.txt")
    with open(path, "w") as fh:
        fh.write(ref.order_file_text(CHROMS, NAMES))
    assert am.read_order_file(path) == GROUPS


def test_config_values_are_replaced_or_added(tmp_path):
    """The written config must carry every one of the further values, also where the input config has no line for a key."""
    from hic_genome_assembler_amd import assembledMap as am
    path = str(tmp_path / "config.txt")
    with open(path, "w", newline="") as fh:
        fh.write("### a comment = kept ###\r\nresolution = 5\nvalidPairFile = /data/pairs\n#originalFastaFile = old\nminSize = 3")
    values = {"hicProScaffSizeFile": "/out/assembly.sizes", "validPairFile": "/dev/null", "restrictionSiteFile": "/dev/null",
              "originalFastaFile": "/out/assembled.fasta"}
    am.set_config_values(path, values)
    with open(path, newline="") as fh:
        text = fh.read()
    assert text == ("### a comment = kept ###\r\nresolution = 5\nvalidPairFile = /dev/null\n#originalFastaFile = old\nminSize = 3\n"
                    "hicProScaffSizeFile = /out/assembly.sizes\nrestrictionSiteFile = /dev/null\noriginalFastaFile = /out/assembled.fasta\n")
    am.set_config_values(path, values)                       # nothing is added twice
    with open(path, newline="") as fh:
        assert fh.read() == text


def test_builder_refusals():
    from hic_genome_assembler_amd import assembledMap as am
    for groups, gap, word in (([[["c", "+"], ["zz", "+"]]], 100, "zz"),
                              ([[["c", "+"], ["c.brk1", "+"]]], 100, "c.brk1"),
                              ([[["c", "+"]], [["a", "-"], ["c", "-"]]], 100, "twice"),
                              ([[["c", "+"], ["c", "+"]]], 100, "twice"),
                              ([[["c", "x"]]], 100, "orientation"),
                              ([[["c", ""]]], 100, "orientation"),
                              ([[["c", "+"]], []], 100, "no scaffold"),
                              ([[]], 100, "no scaffold"),
                              (GROUPS, -1, "negative")):
        with pytest.raises(ValueError) as exc:
            am.build_assembly(groups, NAMES, SIZES, gap)
        assert word in str(exc.value), str(exc.value)


def test_bad_input_is_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import assembledMap as am, synth
    d = str(tmp_path)
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    with open(paths["hicProScaffSizeFile"], "w") as fh:
        fh.write("a\t1000000\nb\t%d\n" % (65535 * 100))
    pairs = os.path.join(d, "pairs.allValidPairs")
    with open(pairs, "wb") as fh:
        fh.write(b"r\ta\t10\t+\tb\t20\n")
    out = str(tmp_path / "assembled")

    def order(text, name):
        path = os.path.join(d, name)
        with open(path, "w") as fh:
            fh.write(text)
        return path

    good = order("### 1 ###\na\t+\nb\t-\n", "good.txt")

    def refused(cfg, word, resolution="1000", order_file=good, more=()):
        with pytest.raises(SystemExit) as exc:
            am.main(["-config", cfg, "-resolution", resolution, "-out", out, "-order", order_file] + list(more))
        assert word in str(exc.value.code) and str(exc.value.code).startswith("ERROR... ") and \
            str(exc.value.code).endswith(" Exiting..."), exc.value.code

    save = os.path.join(d, "save")
    cfg = synth.write_config(os.path.join(d, "config.txt"), paths, save, os.path.join(d, "plots"), 100000,
                             extra={"validPairFile": pairs})
    refused(cfg, "zz", order_file=order("### 1 ###\na\t+\nzz\t+\n", "unknown.txt"))
    refused(cfg, "a.brk1", order_file=order("### 1 ###\na.brk1\t+\na.brk2\t+\n", "broken.txt"))
    refused(cfg, "twice", order_file=order("### 1 ###\na\t+\n### 2 ###\nb\t+\na\t-\n", "twice.txt"))
    refused(cfg, "orientation", order_file=order("### 1 ###\na\t+\nb\t?\n", "orient.txt"))
    refused(cfg, "no scaffold", order_file=order("### 1 ###\na\t+\n### 2 ###\n### 3 ###\nb\t+\n", "empty.txt"))
    refused(cfg, "no scaffold", order_file=order("### 1 ###\na\t+\n### 2 ###\n", "empty_last.txt"))
    refused(cfg, "orientation column", order_file=order("### 1 ###\na\n", "one_column.txt"))
    refused(cfg, "does not exist", order_file=os.path.join(d, "nothing_here"))
    refused(cfg, "negative", more=["-gap", "-1"])
    refused(cfg, "below 1", resolution="0")
    refused(cfg, "below 1", resolution="1000,-3")
    refused(cfg, "twice", resolution="1000,2000,1000")
    # 10,000 + 65,535 bins on the scaffolds ... and the gap between them makes one bin more
    refused(cfg, "resolution 100 needs 75536 bins", resolution="1000,100", more=["-gap", "100"])
    refused(cfg, "resolution 100 needs 75535 bins", resolution="100", more=["-gap", "0"])
    refused(synth.write_config(os.path.join(d, "config2.txt"), paths, save, os.path.join(d, "plots"), 100000), "validPairFile")
    refused(synth.write_config(os.path.join(d, "config3.txt"), paths, save, os.path.join(d, "plots"), 100000,
                               extra={"validPairFile": os.path.join(d, "nothing_here")}), "validPairFile")
    assert not os.path.exists(out) and not os.path.exists(os.path.join(save, "assembled")) and os.listdir(save) == []


# d -> slot, worked by hand from 1 + 4 e + (((d - 2^e) * 4) >> e)
SLOTS = {0: 0, 1: 1, 2: 5, 3: 7, 4: 9, 5: 10, 7: 12, 8: 13, 2 ** 40: 161, 2 ** 40 + 2 ** 38 - 1: 161, 2 ** 40 + 2 ** 38: 162}


def test_slot_formula():
    from hic_genome_assembler_amd import assembledMap as am
    for d, want in SLOTS.items():
        assert ref.slot(d) == want and am.decay_slot(d) == want, d
    assert ref.slot(2 ** 63 - 1) == 252 and ref.slot(2 ** 62) == 249
    # every slot's bounds hold exactly the distances that fall in it
    seen = set()
    for d in list(range(0, 5000)) + [2 ** k + j for k in range(12, 63) for j in (-1, 0, 1)]:
        k = am.decay_slot(d)
        assert k == ref.slot(d) and 0 <= k <= 252
        lo, hi = am.decay_bounds(k)
        assert lo <= d <= hi and am.decay_slot(lo) == am.decay_slot(hi) == k
        assert am.decay_slot(hi + 1) == (k + 1 if am.decay_bounds(k + 1) else am.decay_slot(hi + 1)) > k
        seen.add(k)
    assert am.decay_bounds(2) is None and am.decay_bounds(6) is None and {0, 1, 5, 7, 9, 10, 11, 12, 13} <= seen


def test_header_and_binding_declare_the_exports():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = re.sub(r"\s+", " ", fh.read())
    tables = "const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq"
    outs = "uint64_t *decay_out, uint64_t *seq_cis_out, uint64_t *seq_trans_out, uint64_t *unlifted_out"
    assert "int hicmi_map_begin_lifted(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, " + tables + \
        ", int64_t resolution);" in text
    assert ("int hicmi_pair_stats(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b, "
            "const int64_t *pos_b, int64_t n, const int64_t *scaf_size, int64_t n_scaf, " + tables + ", " + outs + ");") in text
    assert ("int hicmi_lift_maps(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names, "
            "const int64_t *scaf_size, " + tables + ", int64_t n_res, const int64_t *resolution, hicmi_ctx *const *ctxs, "
            "int threads, int64_t *stats5, " + outs + ");") in text
    lib = _lib.load()
    for name, n_args in {"hicmi_map_begin_lifted": 9, "hicmi_pair_stats": 17, "hicmi_lift_maps": 19}.items():
        assert len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
    for method in ("map_begin_lifted", "pair_stats"):
        assert callable(getattr(_lib.Context, method))
    assert callable(_lib.lift_maps) and callable(_lib.new_pair_stats)
    assert lib.hicmi_abi_version() == 1
    # the counting form of a lifted build is read at every call
    with open(os.path.join(CSRC, "api.hip")) as fh:
        api = fh.read()
    assert 'getenv("HICMI_LIFTMAP_PLAIN")' in api
    # ... and it, not buildMap's switch, names the form wherever a lifted build is counted: the two forms give the same
    # bytes, so no test of the results can see which one ran
    assert "c->map_lift.seq ? liftmap_plain() : buildmap_plain()" in api and "lift ? liftmap_plain() : buildmap_plain()" in api
    assert api.count("buildmap_plain()") == 3 and api.count("liftmap_plain()") == 3          # a definition and two uses each
    assert not [ln for ln in api.splitlines() if "HICMI_LIFTMAP_PLAIN" in ln and re.search(r"\bstatic\b[^;]*\bgetenv\(", ln)]


# ---- the native lift, key, slot and table check as host code under the sanitizers -------------------------------------------
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("liftmap") / "liftmap_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "liftmap_host_check.cpp"), "-o", exe])

    def run(path, sizes, tables, r, pairs, distances):
        seq, off, rev, seq_sizes = tables
        lines = ["T %d %d %d" % (len(sizes), len(seq_sizes), r)]
        lines += ["%d %d %d %d" % row for row in zip(map(int, sizes), map(int, seq), map(int, off), map(int, rev))]
        lines += [" ".join(str(int(x)) for x in seq_sizes), "P %d" % len(pairs)]
        lines += ["%d %d %d %d" % tuple(p) for p in pairs]
        lines += ["D %d" % len(distances)] + [str(int(x)) for x in distances]
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
        done = subprocess.run([exe, path], capture_output=True, text=True)
        assert done.returncode == 0 and done.stderr == "", done.stderr
        return done.stdout.splitlines()
    return run


def _expected_pair_lines(sizes, tables, r, pairs):
    first, m = ref.bref.first_bins(tables[3], r)
    out = []
    for sa, pa, sb, pb in pairs:
        qa, xa = ref.lift_one(tables, sizes, sa, pa)
        qb, xb = ref.lift_one(tables, sizes, sb, pb)
        key = -1
        if qa >= 0 and qb >= 0:
            i, j = int(first[qa]) + (xa - 1) // r, int(first[qb]) + (xb - 1) // r
            key = min(i, j) * m + max(i, j)
        out.append("pair %d %d %d %d %d" % (qa, xa, qb, xb, key))
    return out


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("gap", sorted(HAND))
def test_native_lift_and_key_under_the_sanitizers(gap, drop, host_check, tmp_path):
    tables = ref.layout(CHROMS, SIZES, gap, drop_unplaced=drop)
    ends = [(s, p) for s in range(5) for p in range(1, int(SIZES[s]) + 1)]
    pairs = [a + b for a in ends for b in ends]                               # every end against every end: 400 pairs
    for r in (1, 2, 3, 1000):
        got = host_check(str(tmp_path / "case.txt"), SIZES, tables, r, pairs, sorted(SLOTS))
        assert got[0] == "check 0 "
        assert got[1:1 + len(pairs)] == _expected_pair_lines(SIZES, tables, r, pairs)
        assert got[1 + len(pairs):] == ["slot %d" % SLOTS[d] for d in sorted(SLOTS)]


def test_native_64_bit_lift_under_the_sanitizers(host_check, tmp_path):
    sizes = np.array([2 ** 33] * 3 + [5], dtype=np.int64)
    tables = ref.layout([[(0, "+"), (1, "-"), (2, "+")]], sizes, 100)
    assert tables[3].tolist() == [3 * 2 ** 33 + 200, 5]
    edge = [1, 2, 2 ** 27, 2 ** 27 + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 33 - 1, 2 ** 33]
    ends = [(s, p) for s in range(3) for p in edge] + [(3, 1), (3, 5)]
    pairs = [a + b for a in ends for b in ends]
    distances = [2 ** 62, 2 ** 62 + 2 ** 60 - 1, 2 ** 62 + 2 ** 60, 2 ** 63 - 1, 2 ** 32 - 1, 2 ** 32, 3 * 2 ** 33 + 199]
    for r in (2 ** 27, 2 ** 32, 2 ** 32 + 1, 2 ** 35):
        got = host_check(str(tmp_path / "case.txt"), sizes, tables, r, pairs, distances)
        assert got[0] == "check 0 "
        assert got[1:1 + len(pairs)] == _expected_pair_lines(sizes, tables, r, pairs)
        assert got[1 + len(pairs):] == ["slot %d" % ref.slot(d) for d in distances]


def test_native_table_check_under_the_sanitizers(host_check, tmp_path):
    good = ref.layout(CHROMS, SIZES, 1)
    big = 2 ** 63 - 1

    def verdict(sizes=SIZES, seq=None, off=None, seq_sizes=None):
        tables = (good[0] if seq is None else np.asarray(seq, np.int32), good[1] if off is None else np.asarray(off, np.int64),
                  good[2], good[3] if seq_sizes is None else np.asarray(seq_sizes, np.int64))
        return host_check(str(tmp_path / "case.txt"), np.asarray(sizes, np.int64), tables, 2, [(0, 1, 0, 1)], [])[0]

    assert verdict() == "check 0 "
    assert verdict(seq=[0, 0, 0, 1, 3]).startswith("check -1 scaffold 4 lies in sequence 3")
    assert verdict(seq=[0, -2, 0, 1, 2]).startswith("check -1 scaffold 1 lies in sequence -2")
    assert verdict(off=[10, -1, 0, 0, 0]).startswith("check -1 scaffold 1 has the negative offset -1")
    assert verdict(off=[11, 8, 0, 0, 0]).startswith("check -1 scaffold 0 ")                       # 11 + 5 > 15
    assert verdict(off=[10, 8, 0, 0, 1]).startswith("check -1 scaffold 4 ")                       # 1 + 4 > 4
    assert verdict(off=[big, 8, 0, 0, 0]).startswith("check -1 scaffold 0 ")                      # no overflow in off + size
    assert verdict(sizes=[5, 1, big, 3, 4], seq_sizes=[big, 3, 4], off=[0, 8, 0, 0, 0]).startswith("check -1 scaffolds ")
    assert verdict(off=[10, 6, 0, 0, 0]) == "check -1 scaffolds 2 and 1 overlap in sequence 0"    # b inside c
    assert verdict(off=[7, 8, 0, 0, 0]) == "check -1 scaffolds 0 and 1 overlap in sequence 0"     # a over b and the gap
    assert verdict(sizes=[5, 0, 7, 3, 4], off=[10, 3, 0, 0, 0]) == "check 0 "                       # a scaffold of size 0 overlaps nothing
    assert verdict(sizes=[5, 1, -7, 3, 4]).startswith("check -1 scaffold 2 has the negative size")
    assert verdict(seq_sizes=[15, -3, 4]).startswith("check -1 sequence 1 has the negative size")
    assert verdict(seq=[0, 0, 0, 1, -1]) == "check 0 "                                             # a dropped scaffold is not looked at
    assert verdict(seq=[0, 0, 0, 1, -1], off=[10, 8, 0, 0, -5]) == "check 0 "
