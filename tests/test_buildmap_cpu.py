"""buildMap without a GPU: the bin grid, the chunked valid-pair parser against the plain-Python parser of
tests/buildmap_reference.py, the refusals of the command line, synth.write_valid_pairs as the inverse of the reference
builder, and the declarations.  Every comparison is exact: the counts are integers."""
import functools
import os
import re

import numpy as np
import pytest

import buildmap_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = ref.R


# ---- the grid ----------------------------------------------------------------------------------------------------------
def test_bins_from_sizes_edge_sizes(tmp_path):
    from hic_genome_assembler_amd import hostio
    sizes = [1, R - 1, R, R + 1, 3 * R + 7]
    names = ["s%d" % k for k in range(5)]
    bins = hostio.bins_from_sizes((names, sizes), R)
    per = [[b for b in bins if b.chrom == n] for n in names]
    assert [len(p) for p in per] == [1, 1, 1, 2, 4]
    assert [p[-1].stop for p in per] == sizes
    assert [(b.chrom, b.start, b.stop, b.ID) for b in bins] == ref.bed_rows(names, sizes, R)
    assert [b.ID for b in bins] == list(range(1, 10)) and hostio.count_bins(sizes, R) == 9
    assert (per[4][3].start, per[4][3].stop) == (3 * R, 3 * R + 7) and (per[3][1].start, per[3][1].stop) == (R, R + 1)
    # the same grid from the file
    size_file = str(tmp_path / "g.sizes")
    with open(size_file, "w") as fh:
        fh.write("".join("%s\t%d\n" % ns for ns in zip(names, sizes)))
    again = hostio.bins_from_sizes(size_file, R)
    assert [(b.chrom, b.start, b.stop, b.ID) for b in again] == [(b.chrom, b.start, b.stop, b.ID) for b in bins]
    with pytest.raises(ValueError):
        hostio.bins_from_sizes((names, sizes), 0)
    with open(size_file, "a") as fh:
        fh.write("s2\t5\n")
    with pytest.raises(ValueError):
        hostio.read_scaffold_sizes(size_file)


@pytest.mark.parametrize("k", [2, 3, 5])
def test_grid_at_k_r_is_rebin_bins_of_the_grid_at_r(k, tmp_path):
    from hic_genome_assembler_amd import hostio
    names, sizes = ref.odd_scaffolds()
    fine = hostio.bins_from_sizes((names, sizes), R)
    coarse, group_start = hostio.rebin_bins(fine, k)
    direct = hostio.bins_from_sizes((names, sizes), k * R)
    assert [(b.chrom, b.start, b.stop, b.ID) for b in direct] == [(b.chrom, b.start, b.stop, b.ID) for b in coarse]
    assert len(direct) == ref.first_bins(sizes, k * R)[1] == len(group_start) - 1
    a, b = str(tmp_path / "a.bed"), str(tmp_path / "b.bed")
    hostio.write_bed(a, direct)
    hostio.write_bed(b, coarse)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()


# ---- the parser --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _odd_file():
    names, sizes = ref.odd_scaffolds()
    data = ref.odd_file_bytes(names, sizes, 3000, seed=11)
    pairs, stats, after = ref.parse_text(data, names, sizes)
    for a in pairs:
        a.setflags(write=False)
    return names, sizes, data, pairs, stats, after


def _write(tmp_path, data, name="pairs.allValidPairs"):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return path


def test_the_odd_file_has_its_oddities():
    names, sizes, data, pairs, stats, _after = _odd_file()
    assert data.count(b"\r\n") > 100 and not data.endswith(b"\n")
    cols = {ln.rstrip(b"\r").count(b"\t") + 1 for ln in data.split(b"\n")}
    assert cols == {6, 12}
    lines, used, unknown, out_of_range = stats
    assert lines == 3000 and unknown > 100 and out_of_range > 100 and used == lines - unknown - out_of_range
    sa, pa, sb, pb = pairs
    assert (pa == 1).any() and (pb == sizes[sb]).any() and (pa == sizes[sa]).any()


@pytest.mark.parametrize("threads", [1, 3, 16])
@pytest.mark.parametrize("max_pairs", [1, 7, 1000, 10 ** 6, None])
def test_parser_matches_the_python_parser(threads, max_pairs, tmp_path):
    """One call, and the whole file walked by next_byte: pairs, statistics and every stop."""
    from hic_genome_assembler_amd import _lib
    names, sizes, data, want, stats, after = _odd_file()
    path = _write(tmp_path, data)
    got = [[], [], [], []]
    total = np.zeros(4, np.int64)
    pos, calls = 0, 0
    while True:
        sa, pa, sb, pb, nxt, st = _lib.parse_valid_pairs(path, names, sizes, first_byte=pos, max_pairs=max_pairs, threads=threads)
        calls += 1
        assert sa.dtype == np.int32 and pa.dtype == np.int64 and st[1] == len(sa)
        for dst, src in zip(got, (sa, pa, sb, pb)):
            dst.append(src.copy())
        total += st
        n_so_far = sum(len(x) for x in got[0])
        if max_pairs is not None and len(sa) == max_pairs:
            assert nxt == after[n_so_far - 1]                            # right after the line of the last pair wanted
        else:
            assert nxt == len(data)
        assert nxt > pos or nxt == len(data)
        pos = nxt
        if pos == len(data):
            break
    assert tuple(total) == stats
    for dst, ref_arr in zip(got, want):
        assert np.concatenate(dst).tobytes() == ref_arr.tobytes()
    if max_pairs in (10 ** 6, None):
        assert calls == 1
    elif max_pairs == 7:
        assert calls >= stats[1] // 7


def test_parser_on_small_files(tmp_path):
    from hic_genome_assembler_amd import _lib
    names, sizes = ["a", "b"], [10, 20]
    empty = _write(tmp_path, b"", "empty")
    sa, pa, sb, pb, nxt, st = _lib.parse_valid_pairs(empty, names, sizes)
    assert len(sa) == len(pa) == len(sb) == len(pb) == 0 and nxt == 0 and st == (0, 0, 0, 0)
    one = _write(tmp_path, b"r\ta\t10\t+\tb\t20", "one")
    sa, pa, sb, pb, nxt, st = _lib.parse_valid_pairs(one, names, sizes, threads=16)
    assert (sa.tolist(), pa.tolist(), sb.tolist(), pb.tolist()) == ([0], [10], [1], [20]) and nxt == 13 and st == (1, 1, 0, 0)
    sa, _pa, _sb, _pb, nxt, st = _lib.parse_valid_pairs(one, names, sizes, first_byte=13)
    assert len(sa) == 0 and nxt == 13 and st == (0, 0, 0, 0)
    with pytest.raises(_lib.HicmiError):
        _lib.parse_valid_pairs(one, names, sizes, first_byte=14)
    with pytest.raises(_lib.HicmiError):
        _lib.parse_valid_pairs(str(tmp_path / "missing"), names, sizes)
    # the longer name is not its prefix, and an unknown name is counted whichever column it is in
    mixed = _write(tmp_path, b"r\tab\t1\t+\ta\t1\nr\ta\t1\t+\tab\t1\nr\tb\t21\t-\ta\t1\nr\tb\t20\t-\ta\t0\r\n", "mixed")
    sa, _pa, _sb, _pb, nxt, st = _lib.parse_valid_pairs(mixed, names, sizes)
    assert len(sa) == 0 and st == (4, 0, 2, 2) and nxt == os.path.getsize(mixed)


@pytest.mark.parametrize("bad", [b"r\ta\t1\t+\tb", b"r\ta\t1\t+\tb\t12x", b"r\ta\tx\t+\tb\t12", b"", b"r\tzz\t1\t+\tzz\t1.5\t-"])
@pytest.mark.parametrize("threads", [1, 16])
def test_malformed_line_is_einval_with_its_offset(bad, threads, tmp_path):
    from hic_genome_assembler_amd import _lib
    names, sizes, data, _want, _stats, _after = _odd_file()
    head = data[:data.index(b"\n", len(data) // 2) + 1]
    path = _write(tmp_path, head + bad + b"\n" + data[len(head):])
    with pytest.raises(ref.Malformed) as py:
        ref.parse_text(head + bad + b"\n" + data[len(head):], names, sizes)
    assert py.value.offset == len(head)
    with pytest.raises(_lib.HicmiError) as exc:
        _lib.parse_valid_pairs(path, names, sizes, threads=threads)
    assert "error -1:" in str(exc.value) and str(exc.value).endswith("at byte %d" % len(head))
    # a call that stops before the line does not see it
    sa, _pa, _sb, _pb, nxt, _st = _lib.parse_valid_pairs(path, names, sizes, max_pairs=50, threads=threads)
    assert len(sa) == 50 and nxt < len(head)
    # ... even when it is inside the bytes the call looked at: the pairs before it, all of them and one more
    n_before = ref.parse_text(head, names, sizes)[1][1]
    sa, _pa, _sb, _pb, nxt, _st = _lib.parse_valid_pairs(path, names, sizes, max_pairs=n_before, threads=threads)
    assert len(sa) == n_before and nxt <= len(head)
    with pytest.raises(_lib.HicmiError):
        _lib.parse_valid_pairs(path, names, sizes, max_pairs=n_before + 1, threads=threads)


# ---- the inverse ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sort", [True, False])
def test_write_valid_pairs_is_the_inverse_of_the_builder(sort, tmp_path):
    from hic_genome_assembler_amd import synth
    lay = synth.make_layout(160, seed=3)
    counts, lay = synth.make_raw_counts(lay, seed=3, depth=20.0)
    path = str(tmp_path / "pairs.allValidPairs")
    n = synth.write_valid_pairs(path, lay, counts, seed=5, sort=sort)
    assert n == np.triu(counts).sum()
    with open(path, "rb") as fh:
        data = fh.read()
    pairs, stats, _after = ref.parse_text(data, lay.scaffold_names, lay.scaffold_sizes_bp)
    assert stats == (n, n, 0, 0)
    assert ref.build(pairs, lay.scaffold_sizes_bp, lay.resolution).tobytes() == counts.tobytes()
    sa, pa, sb, pb = pairs
    assert (sa > sb).any() and (sa < sb).any()                              # either mate first
    key = [(synth.natural_key(lay.scaffold_names[a]), x) for a, x in zip(sa.tolist(), pa.tolist())]
    assert (key == sorted(key)) == sort
    # and the library's parser reads the same pairs
    from hic_genome_assembler_amd import _lib
    got = _lib.parse_valid_pairs(path, lay.scaffold_names, lay.scaffold_sizes_bp, threads=3)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:4], pairs)) and got[5] == stats


def test_natural_key_orders_like_sort_V():
    from hic_genome_assembler_amd import synth
    names = ["scaffold_10", "scaffold_2", "scaffold_1", "chr2b", "chr10"]
    assert sorted(names, key=synth.natural_key) == ["chr2b", "chr10", "scaffold_1", "scaffold_2", "scaffold_10"]


# ---- the command line ------------------------------------------------------------------------------------------------------
def test_resolution_validation():
    from hic_genome_assembler_amd import buildMap
    assert buildMap.parse_resolutions("100000,150000, 250000") == [100000, 150000, 250000]
    for bad in ("0", "-5", "100,100", "1e5", "", "100,,200", "abc"):
        with pytest.raises(ValueError):
            buildMap.parse_resolutions(bad)


def test_bad_input_is_refused_before_anything_is_written(tmp_path):
    from hic_genome_assembler_amd import buildMap, synth
    d = str(tmp_path)
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    with open(paths["hicProScaffSizeFile"], "w") as fh:
        fh.write("a\t1000000\nb\t%d\n" % (65535 * 100))
    pairs = _write(tmp_path, b"r\ta\t10\t+\tb\t20\n")
    out = str(tmp_path / "build")

    def refused(cfg, resolution, word):
        with pytest.raises(SystemExit) as exc:
            buildMap.main(["-config", cfg, "-resolution", resolution, "-out", out])
        assert word in str(exc.value.code), exc.value.code

    cfg = synth.write_config(os.path.join(d, "config.txt"), paths, os.path.join(d, "save"), os.path.join(d, "plots"), 100000,
                             extra={"validPairFile": pairs})
    refused(cfg, "0", "below 1")
    refused(cfg, "1000,-3", "below 1")
    refused(cfg, "1000,2000,1000", "twice")
    refused(cfg, "1000,99", "resolution 99 needs")                            # 10,102 + 66,197 bins
    refused(cfg, "1000,100", "resolution 100 needs 75535 bins")
    # validPairFile: /dev/null (what write_config sets), and a path that is not there
    refused(synth.write_config(os.path.join(d, "config2.txt"), paths, os.path.join(d, "save"), os.path.join(d, "plots"), 100000),
            "1000", "validPairFile")
    refused(synth.write_config(os.path.join(d, "config3.txt"), paths, os.path.join(d, "save"), os.path.join(d, "plots"), 100000,
                               extra={"validPairFile": os.path.join(d, "nothing_here")}), "1000", "validPairFile")
    assert not os.path.exists(out) and not os.path.exists(os.path.join(d, "save", "build"))


# ---- declarations ----------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_exports():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"\b(hicmi_[a-z0-9_]+)\s*\(", text))
    new = {"hicmi_parse_valid_pairs": 15, "hicmi_map_begin": 4, "hicmi_map_add_pairs": 6, "hicmi_map_finish": 2, "hicmi_build_maps": 10}
    lib = _lib.load()
    for name, n_args in new.items():
        assert name in declared and len(_lib.SIGNATURES[name][1]) == n_args and hasattr(lib, name)
    assert re.search(r"int hicmi_map_begin\(hicmi_ctx \*ctx, const int64_t \*scaf_size, int64_t n_scaf, int64_t resolution\);", text)
    assert re.search(r"int hicmi_map_finish\(hicmi_ctx \*ctx, int64_t \*pairs_out\);", text)
    for method in ("map_begin", "map_add_pairs", "map_finish"):
        assert callable(getattr(_lib.Context, method))
    assert callable(_lib.parse_valid_pairs) and callable(_lib.build_maps)
    assert lib.hicmi_abi_version() == 1


def test_the_pair_path_has_one_chunk_loop_one_staging_step_and_one_switch_reader():
    csrc = os.path.join(ROOT, "hic_genome_assembler_amd", "csrc")
    both = ""
    for name in ("api.hip", "api_pairs.inc"):
        with open(os.path.join(csrc, name)) as fh:
            both += fh.read()
    assert both.count('getenv("HICMI_BUILDMAP_CHUNK_PAIRS")') == 1          # the chunk setting is read in one place
    assert both.count("map_chunk_at(c->d_map_chunk") == 1                    # host arrays are staged in one place
    assert both.count('!strcmp(env, "1")') <= 1                              # no switch reader spelt out beside plain_switch
    assert both.count("static int pair_file_pass(") == 1
    loop = both[both.index("static int build_maps_loop("):both.index("int hicmi_build_maps(")]
    assert "pair_file_pass(" in loop and "hipMemcpyAsync(" not in loop and "fopen(" not in loop
