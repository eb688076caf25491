"""Keeps the ld > n coverage closed without a GPU: every place of csrc/api.hip that hands the contact matrix and its
leading dimension to a kernel or a 2-D copy must be named in adopted_matrix.READERS with a GPU test that runs it on an
adopted matrix with ld > n, and the layouts the GPU tests build must be what they say they are."""
import glob
import os
import re

import numpy as np
import pytest

import adopted_matrix as am

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "hic_genome_assembler_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the table
def test_every_reader_of_the_matrix_has_a_layout_test():
    found = am.matrix_readers(am.api_source())
    assert found, "the scan of csrc/api.hip found no reader at all: the patterns no longer match the source"
    missing, stale = sorted(found - set(am.READERS)), sorted(set(am.READERS) - found)
    assert not missing, "csrc/api.hip reads the contact matrix through %s: add a test with ld > n and name it in " \
                        "adopted_matrix.READERS" % missing
    assert not stale, "adopted_matrix.READERS names %s, which csrc/api.hip no longer calls" % stale


def test_the_scan_sees_kernel_launches_and_the_strided_copy():
    src = """
        launch_row_sums(c->dC, c->ldc, (int)c->n, c->d_np, c->d_seq, 0, 1, c->stream);
        launch_new_stage( c->dC , c->ldc, 3);
        HIPCHK(hipMemcpy2DAsync(c->pin_down, sizeof(double) * (size_t)n, c->dC + (row0 + r) * c->ldc,
                                sizeof(double) * (size_t)c->ldc, w, h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(c->dC, contacts, bytes, hipMemcpyHostToDevice, c->stream));
        launch_widen_f32(d_stage, c->dC, (int64_t)cells, c->stream);
        c->n = n; c->ldc = ld; c->dC = const_cast<double*>(d_contacts);
    """
    assert am.matrix_readers(src) == {"launch_row_sums", "launch_new_stage", "hipMemcpy2DAsync"}


def _gpu_tests():
    names = set()
    for path in glob.glob(os.path.join(TESTS, "test_gpu_*.py")):
        with open(path) as fh:
            text = fh.read()
        assert re.search(r"^pytestmark = pytest\.mark\.gpu", text, re.M) or "@pytest.mark.gpu" in text, path
        names |= {"%s::%s" % (os.path.basename(path), t) for t in re.findall(r"^def (test_\w+)\(", text, re.M)}
    return names


def test_the_named_tests_exist():
    have = _gpu_tests()
    for reader, tests in am.READERS.items():
        assert tests, reader
        for t in tests:
            assert t in have, "%s: %s is not a test of a tests/test_gpu_*.py file" % (reader, t)


def test_switches_the_gpu_tests_flip_in_process_are_read_per_call():
    """The GPU tests set HICMI_SORT_RADIX, HICMI_PRESORT_FROM and HICMI_NO_PRESORT between calls of one process, and run
    HICMI_SORT_LDS in a child: the first three must not be cached in a function-local static, the last one is."""
    static = set()
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        with open(path) as fh:
            for line in fh:
                if re.search(r"\bstatic\b[^;]*\bgetenv\(", line):
                    static |= set(re.findall(r'getenv\("(\w+)"\)', line))
    assert "HICMI_SORT_LDS" in static
    assert not static & {"HICMI_SORT_RADIX", "HICMI_PRESORT_FROM", "HICMI_NO_PRESORT", "HICMI_PRESORT_TIES"}


# ------------------------------------------------------------------------------------------------ the layouts
SIZES = [1, 2, 7, 8, 129, 300]


@pytest.mark.parametrize("n", SIZES)
def test_geometry(n):
    ld, shift, size = am.geometry(n, "odd")
    assert ld % 2 == 1 and n < ld <= n + 2 and shift == 0                 # the smallest odd value above n
    assert {(shift + i * ld) % 2 for i in range(min(n, 2))} == ({0, 1} if n > 1 else {0})
    ld, shift, size = am.geometry(n, "even_shifted")
    assert ld % 2 == 0 and n < ld <= n + 2 and shift == 1                 # the smallest even value above n
    assert all((shift + i * ld) % 2 == 1 for i in range(n))               # no row starts on a 16-byte boundary
    assert am.geometry(n, "wide")[:2] == (n + 61, 0)
    ld, shift, size = am.geometry(n, "block")
    a = am.BLOCK_A
    assert a % 2 == 1 and ld == n + a + 5 and shift == a * ld + a and size == ld * ld
    assert am.geometry(n, "dense") == (n, 0, n * n)
    for layout in am.LAYOUTS + ("dense",):
        ld, shift, size = am.geometry(n, layout)
        assert ld >= n and shift >= 0 and shift + (n - 1) * ld + n <= size
        assert (layout == "dense") == (ld == n)
    with pytest.raises(ValueError):
        am.geometry(n, "diagonal")


@pytest.mark.parametrize("poison", ["nan", "finite"])
@pytest.mark.parametrize("layout", am.LAYOUTS + ("dense",))
@pytest.mark.parametrize("n", SIZES)
def test_store_holds_the_matrix_and_poison_everywhere_else(n, layout, poison):
    import torch
    M = np.random.default_rng(n).random((n, n)) + 1.0
    ld, shift, size = am.geometry(n, layout)
    store, view = am.build_store(M, layout, poison, "cpu")
    assert store.dtype == torch.float64 and store.shape == (size,)
    assert view.shape == (n, ld) and view.stride() == (ld, 1) and view.storage_offset() == shift
    assert view.data_ptr() == store.data_ptr() + 8 * shift                # shares the store's memory
    flat = store.numpy()
    cell = np.zeros(size, bool)
    for i in range(n):
        assert np.array_equal(flat[shift + i * ld: shift + i * ld + n], M[i])
        cell[shift + i * ld: shift + i * ld + n] = True
    assert cell.sum() == n * n
    outside = flat[~cell]
    if poison == "nan":
        assert np.all(np.isnan(outside))
    else:
        assert np.array_equal(outside, np.flatnonzero(~cell) + am.FINITE_BASE)      # distinct, far above the contacts
        assert len(outside) == 0 or outside.min() >= am.FINITE_BASE > 1000 * M.max()
    if layout == "block":
        a = am.BLOCK_A
        big = store.view(ld, ld)
        assert np.array_equal(big[a:a + n, a:a + n].numpy(), M)
        assert big[a:a + n, a:a + n].data_ptr() == view.data_ptr()


def test_a_changed_store_is_noticed():
    """The comparison is on the bits: a NaN store equals its snapshot, and one flipped payload bit is seen."""
    import torch
    store, _view = am.build_store(np.ones((3, 3)), "wide", "nan", "cpu")
    snap = store.view(torch.int64).clone()
    assert not torch.equal(store, store.clone())                          # NaN != NaN as floats
    am.assert_untouched(store, snap)
    store.view(torch.int64)[5] ^= 1
    with pytest.raises(AssertionError):
        am.assert_untouched(store, snap)
