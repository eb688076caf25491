"""Part 0 (ICE balancing) without a GPU: the mask rules, the config keys and -part0's refusals, the two
writers, the declarations - and the sanity of tests/ice_reference.py, which the GPU tests compare the device against."""
import os
import re

import numpy as np
import pytest

import ice_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- mask rules (a)-(c) ---------------------------------------------------------------------------------------------
def _mask(w, short=None, p=0.02):
    from hic_genome_assembler_amd import iceNormalize
    return iceNormalize.build_mask(np.asarray(w, dtype=np.float64), None if short is None else np.asarray(short), p)


def test_mask_threshold_index_is_int_n_p():
    w = np.arange(1, 101, dtype=np.float64)[::-1].copy()              # 100 ... 1
    mask, n_a, n_b, n_c = _mask(w, p=0.02)                            # x[int(100 * 0.02)] = x[2] = 3: w < 3 goes
    assert (n_a, n_b, n_c) == (0, 0, 2) and sorted(w[mask]) == [1., 2.]
    mask, _a, _b, n_c = _mask(w[:49], p=0.02)                         # int(49 * 0.02) = 0: x[0] is the minimum, nothing is below
    assert n_c == 0 and not mask.any()
    mask, _a, _b, n_c = _mask(w[:50], p=0.02)                         # int(50 * 0.02) = 1: only the minimum is below x[1]
    assert n_c == 1 and w[:50][mask].tolist() == [51.]
    mask, _a, _b, n_c = _mask(w, p=0.995)                             # int(99.5) = 99: everything but the maximum
    assert n_c == 99 and w[~mask].tolist() == [100.]


def test_mask_ties_at_the_threshold_stay():
    w = np.array([5., 1., 5., 5., 9., 5., 7., 8., 5., 6.])
    mask, _a, _b, n_c = _mask(w, p=0.3)                               # sorted: 1 5 5 5 5 5 6 7 8 9; x[3] = 5; only w < 5
    assert n_c == 1 and np.flatnonzero(mask).tolist() == [1]
    mask, _a, _b, n_c = _mask(w, p=0.6)                               # x[6] = 6: all the fives go together
    assert n_c == 6 and np.flatnonzero(mask).tolist() == [0, 1, 2, 3, 5, 8]


def test_mask_zero_bins_and_p_zero():
    w = np.array([0., 4., 0., 2., 3., 0., 9., 8.])
    mask, n_a, n_b, n_c = _mask(w, p=0.0)
    assert (n_a, n_b, n_c) == (0, 3, 0) and np.flatnonzero(mask).tolist() == [0, 2, 5]
    # the zero bins are part of the sorted weights: x = 0 0 0 2 3 4 8 9, int(8 * 0.5) = 4, threshold 3
    mask, n_a, n_b, n_c = _mask(w, p=0.5)
    assert (n_a, n_b, n_c) == (0, 3, 1) and np.flatnonzero(mask).tolist() == [0, 2, 3, 5]
    # rule (a) first: its bins arrive with weight 0 (their rows are zeroed) and are counted under (a)
    mask, n_a, n_b, n_c = _mask(w, short=[True, False, False, False, False, False, False, False], p=0.0)
    assert (n_a, n_b, n_c) == (1, 2, 0)
    assert _mask(np.zeros(4), p=0.02)[0].all()


@pytest.mark.parametrize("n", [5, 64, 257])
def test_mask_agrees_with_the_reference(n):
    from hic_genome_assembler_amd import iceNormalize
    counts, _lay, short = ref.make_case(n)
    c = counts.copy()
    if short is not None:
        c[short, :] = 0.0
        c[:, short] = 0.0
    for p in (0.0, 0.02, 0.2):
        got = iceNormalize.build_mask(c.sum(axis=1), short, p)
        want = ref.ice_mask(counts, short, p)
        assert np.array_equal(got[0], want[0]) and tuple(got[1:]) == tuple(want[1:])
    if n == 257:
        assert want[1] >= 2                                            # the two short scaffolds


def test_short_scaffold_bins(tmp_path):
    from hic_genome_assembler_amd import hostio, iceNormalize, synth
    counts, lay, short = ref.make_case(257)
    paths = synth.write_hicpro(str(tmp_path), lay, None, raw_counts=counts)
    bins = hostio.read_bed_bins(paths["hicProBedFile"])
    assert [b.ID for b in bins] == lay.bin_ids.tolist() and len(bins) == 257
    got = iceNormalize.short_scaffold_bins(bins, paths["hicProScaffSizeFile"], ref.MIN_SCAFFOLD_SIZE)
    assert np.array_equal(got, short) and 2 <= got.sum() < 257
    assert not iceNormalize.short_scaffold_bins(bins, paths["hicProScaffSizeFile"], 1).any()
    # the raw file holds the counts: integer triplets of the upper triangle
    back = hostio.read_contact_matrix(paths["hicProRawMatrixFile"], bins, engine="pandas")
    assert np.array_equal(back, counts)


# ---- config keys and -part0's refusals ------------------------------------------------------------------------------
def _config(tmp_path, extra=None):
    from hic_genome_assembler_amd import synth
    d = str(tmp_path)
    paths = {k: os.path.join(d, k + ".txt") for k in ("hicProBedFile", "hicProBiasFile", "hicProMatrixFile", "hicProScaffSizeFile")}
    return synth.write_config(os.path.join(d, "config.txt"), paths, os.path.join(d, "save"), os.path.join(d, "plots"), 100000,
                              extra=extra), paths


def test_config_without_the_keys_is_unchanged(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as drv
    cfg, _paths = _config(tmp_path)
    v = drv.readConfigFileToVariables(cfg)
    assert set(v) == {k for k, _d, _kind, _p in drv._SPEC}              # no new key appears unless the file sets it
    assert not drv.ensureAllVariablesAreSet(v)


def test_config_keys_are_parsed(tmp_path):
    from hic_genome_assembler_amd import run_hicAssembler as drv
    cfg, _paths = _config(tmp_path, extra={"hicProRawMatrixFile": "/data/sample_100000.matrix", "iceFilterLowPerc": "0.05",
                                           "iceMaxIter": "250", "iceEps": "1e-3", "iceMinScaffoldSize": "10000"})
    v = drv.readConfigFileToVariables(cfg)
    assert v["hicProRawMatrixFile"] == "/data/sample_100000.matrix"      # a full path: no directory is put in front
    assert v["iceFilterLowPerc"] == 0.05 and v["iceMaxIter"] == 250 and v["iceEps"] == 1e-3 and v["iceMinScaffoldSize"] == 10000
    assert isinstance(v["iceMaxIter"], int) and isinstance(v["iceMinScaffoldSize"], int)
    raw, ice = drv.part0Settings(v)
    assert raw == "/data/sample_100000.matrix"
    assert ice == {"iceFilterLowPerc": 0.05, "iceMaxIter": 250, "iceEps": 1e-3, "iceMinScaffoldSize": 10000}
    cfg, _paths = _config(tmp_path, extra={"hicProRawMatrixFile": "/data/raw.matrix", "iceMaxIter": "many"})
    v = drv.readConfigFileToVariables(cfg)
    assert "iceMaxIter" not in v
    assert drv.part0Settings(v)[1] == {"iceFilterLowPerc": 0.02, "iceMaxIter": 100, "iceEps": 0.1, "iceMinScaffoldSize": None}


def test_part0_without_raw_matrix_exits_with_the_message(tmp_path, capsys):
    from hic_genome_assembler_amd import run_hicAssembler as drv
    cfg, _paths = _config(tmp_path)
    with pytest.raises(SystemExit) as exc:
        drv.main(["-part0", "-config", cfg])
    assert "hicProRawMatrixFile" in str(exc.value.code) and "-part0" in str(exc.value.code)
    from hic_genome_assembler_amd import iceNormalize
    with pytest.raises(SystemExit) as exc:
        iceNormalize.main(["-config", cfg])
    assert "hicProRawMatrixFile" in str(exc.value.code)


@pytest.mark.parametrize("key", ["hicProMatrixFile", "hicProBiasFile"])
def test_part0_refuses_raw_equal_to_an_output(tmp_path, key):
    from hic_genome_assembler_amd import run_hicAssembler as drv
    cfg, paths = _config(tmp_path)
    with open(paths[key], "w") as fh:
        fh.write("1\t1\t5\n")
    # the same file under another name: through a symbolic link and through a path with ..
    link = os.path.join(str(tmp_path), "raw.matrix")
    os.symlink(paths[key], link)
    for raw in (paths[key], link, os.path.join(str(tmp_path), "save", "..", os.path.basename(paths[key]))):
        cfg, _p = _config(tmp_path, extra={"hicProRawMatrixFile": raw})
        with pytest.raises(SystemExit) as exc:
            drv.main(["-part0", "-config", cfg])
        assert key in str(exc.value.code) and "same file" in str(exc.value.code)
        with open(paths[key]) as fh:
            assert fh.read() == "1\t1\t5\n"                             # nothing was written


# ---- writers --------------------------------------------------------------------------------------------------------
def test_writers_round_trip_bit_for_bit(tmp_path):
    from hic_genome_assembler_amd import hostio, synth
    counts, lay, short = ref.make_case(65)
    mask = ref.ice_mask(counts, short)[0]
    mask[[3, 40]] = True
    X, bias, _it, _dl, _dls = ref.ice_balance(counts, mask, 100, 1e-6)
    X = 0.5 * (X + X.T)                                                 # the device's result is exactly symmetric
    paths = synth.write_hicpro(str(tmp_path), lay, None)
    mfile, bfile = os.path.join(str(tmp_path), "iced.matrix"), os.path.join(str(tmp_path), "iced.biases")
    hostio.write_biases(bfile, bias)
    hostio.write_iced_matrix(mfile, X, lay.bin_ids)
    with open(bfile) as fh:
        lines = fh.read().split("\n")
    assert lines[-1] == "" and len(lines) == 65 + 1                     # one line per bed line
    assert [i for i, t in enumerate(lines[:-1]) if t == "nan"] == np.flatnonzero(mask).tolist()
    assert all(float(t) == b for t, b in zip(lines[:-1], bias.tolist()) if t != "nan")
    with open(mfile) as fh:
        trip = [ln.split("\t") for ln in fh.read().splitlines()]
    keys = [(int(a), int(b)) for a, b, _v in trip]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)          # row, then column, ascending
    assert all(a <= b for a, b in keys)                                  # upper triangle with the diagonal
    assert any(a == b for a, b in keys)
    assert len(keys) == int(np.count_nonzero(np.triu(X)))                # non-zero values only, all of them
    assert all(float(v) != 0.0 and v == repr(float(v)) for _a, _b, v in trip)
    # the loaders of Parts 1 and 2: the masked bins are gone, the rest is X to the last bit
    bins = hostio.initiateLoci(paths["hicProBedFile"], bfile)
    keep = np.flatnonzero(~mask)
    assert [b.ID for b in bins] == lay.bin_ids[keep].tolist()
    assert [b.bias for b in bins] == bias[keep].tolist()
    back = hostio.read_contact_matrix(mfile, bins, engine="pandas")
    assert back.tobytes() == np.ascontiguousarray(X[np.ix_(keep, keep)]).tobytes()
    assert hostio.read_contact_matrix(mfile, bins).tobytes() == back.tobytes()      # the native parser too


def test_native_writer_writes_what_repr_writes(tmp_path):
    from hic_genome_assembler_amd import _lib, hostio
    rng = np.random.default_rng(5)
    special = [1e16, 1e15, 9999999999999998.0, 1.5e16, 1e22, 1e100, 1.7976931348623157e308, 5e-324, 2.2250738585072014e-308,
               1e-4, 1e-5, 0.00012345, 9.999e-5, 0.1, 0.3, 1.0, 2.0, 100.0, 123456.789, 1 / 3, 2 / 3, 1e-7 / 3, 4.35, 0.5, 1e23,
               123456789012345680.0, 12345678901234567.0, 1234567890123456.7, -2.5, -1e-10, float("inf"), float("nan")]
    values = special + (rng.random(2000) * 10.0 ** rng.integers(-12, 20, 2000)).tolist() + rng.integers(1, 10 ** 6, 500).astype(float).tolist()
    for v in values:
        assert _lib.format_double(v) == repr(float(v))
    # a whole file: 70 bins (more than one work item of rows), zeros skipped, both engines byte for byte
    n = 70
    m = rng.random((n, n)) * 10.0 ** rng.integers(-8, 8, (n, n))
    m[rng.random((n, n)) < 0.4] = 0.0
    m = np.triu(m) + np.triu(m, 1).T
    m[17, :] = 0.0
    m[:, 17] = 0.0
    ids = np.arange(1001, 1001 + n) * 7
    a, b = str(tmp_path / "native.matrix"), str(tmp_path / "python.matrix")
    hostio.write_iced_matrix(a, m, ids)
    hostio.write_iced_matrix(b, m, ids, engine="python")
    with open(a, "rb") as fa, open(b, "rb") as fb:
        text = fa.read()
        assert text == fb.read()
    assert text.count(b"\n") == int(np.count_nonzero(np.triu(m))) == _lib.write_hicpro_matrix(a, m, ids, threads=3)
    with open(a, "rb") as fa:
        assert fa.read() == text
    with pytest.raises(_lib.HicmiError):
        _lib.write_hicpro_matrix(str(tmp_path / "no" / "such" / "dir.matrix"), m, ids)


# ---- the reference itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 257])
def test_reference_converges_to_equal_row_sums(n):
    counts, _lay, short = ref.make_case(n)
    mask, _a, n_b, _c = ref.ice_mask(counts, short)
    assert n_b == 1                                                      # the dead bin
    X, bias, iters, delta, deltas = ref.ice_balance(counts, mask, 1000, 1e-6)
    assert 1 < iters < 1000 and delta < 1e-6 and len(deltas) == iters - 1
    s = X.sum(axis=1)[~mask]
    assert (s.max() - s.min()) / s.mean() < 1e-6
    assert np.isnan(bias[mask]).all() and np.isfinite(bias[~mask]).all()
    assert not X[mask, :].any() and not X[:, mask].any()
    # X = C / (bias_i bias_j) on the unmasked bins, and the total is kept
    k = np.flatnonzero(~mask)
    C = counts[np.ix_(k, k)]
    assert np.allclose(X[np.ix_(k, k)], C / np.outer(bias[k], bias[k]), rtol=1e-12, atol=0)
    assert X.sum() == pytest.approx(C.sum(), rel=1e-12)


def test_reference_ends_at_max_iter_without_error():
    counts, _lay, short = ref.make_case(63)
    mask = ref.ice_mask(counts, short)[0]
    _X, _bias, iters, delta, deltas = ref.ice_balance(counts, mask, 7, 1e-12)
    assert iters == 7 and delta > 1e-12 and len(deltas) == 6
    assert ref.stop_margin(deltas, 1e-12) > 1.0


# ---- declarations ---------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_exports():
    from hic_genome_assembler_amd import _lib
    with open(os.path.join(ROOT, "include", "hicmi.h")) as fh:
        text = fh.read()
    declared = set(re.findall(r"\b(hicmi_[a-z0-9_]+)\s*\(", text))
    assert {"hicmi_ice_mask_rows", "hicmi_ice_balance"} <= declared
    assert {"hicmi_ice_mask_rows", "hicmi_ice_balance"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["hicmi_ice_balance"][1]) == 7 and len(_lib.SIGNATURES["hicmi_ice_mask_rows"][1]) == 3
    for name in ("ice_mask_rows", "ice_balance"):
        assert callable(getattr(_lib.Context, name))
