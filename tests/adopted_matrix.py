"""Contact matrices the library adopts from the caller (hicmi_set_contacts_device) with a leading dimension above n.

``adopt`` lays a host matrix out in a flat fp64 store - padded rows, a base that is not 16-byte aligned, or a square
block of a larger map - fills every cell outside the n x n matrix with poison and hands the view to a context.
``assert_untouched`` compares the store with its snapshot bit for bit: an adopted source is only ever read.
``READERS`` names every place of csrc/api.hip that reads the contact matrix and the GPU tests that run it with ld > n
(tests/test_adopted_cpu.py keeps the table and the source in step)."""
import os
import re

import numpy as np

LAYOUTS = ("odd", "even_shifted", "wide", "block")
BLOCK_A = 3                     # the block layout is big[a:a + n, a:a + n] of an (n + a + 5)-square store; a is odd
FINITE_BASE = 3.0e5             # finite poison: FINITE_BASE + flat index, a different large value in every cell


def geometry(n, layout):
    """(ld, shift, store elements) of ``layout`` for an n x n matrix: cell (i, j) is store[shift + i * ld + j]."""
    if layout == "dense":
        return n, 0, n * n
    if layout == "odd":                                    # rows alternate between 16- and 8-byte alignment
        ld = n + 1 if n % 2 == 0 else n + 2
        return ld, 0, n * ld
    if layout == "even_shifted":                           # no row is 16-byte aligned
        ld = n + 2 if n % 2 == 0 else n + 1
        return ld, 1, n * ld + 2
    if layout == "wide":
        return n + 61, 0, n * (n + 61)
    if layout == "block":
        ld = n + BLOCK_A + 5
        return ld, BLOCK_A * ld + BLOCK_A, ld * ld
    raise ValueError("unknown layout " + repr(layout))


def build_store(M, layout, poison, device):
    """(store, view): the flat store of ``layout`` filled with ``poison`` ("nan" or "finite") and its strided n x ld
    view, M copied into view[:, :n].  Works on any torch device (the index arithmetic is unit-tested on the CPU)."""
    import torch
    M = np.ascontiguousarray(M, dtype=np.float64)
    n = M.shape[0]
    assert M.shape == (n, n) and n >= 1
    ld, shift, size = geometry(n, layout)
    assert ld >= n and shift + n * ld <= size
    if poison == "nan":
        store = torch.full((size,), float("nan"), dtype=torch.float64, device=device)
    elif poison == "finite":
        store = torch.arange(size, dtype=torch.float64, device=device) + FINITE_BASE
    else:
        raise ValueError("poison must be 'nan' or 'finite'")
    view = store[shift:shift + n * ld].view(n, ld)
    view[:, :n] = torch.as_tensor(M, device=device)
    return store, view


def adopt(ctx, M, layout, poison="nan"):
    """Hand M to ``ctx`` as an adopted device matrix in ``layout``; returns (store, bit snapshot of the store)."""
    import torch
    n = len(M)
    ld, shift, _size = geometry(n, layout)
    store, view = build_store(M, layout, poison, "cuda:0")
    assert store.data_ptr() % 16 == 0 and view.data_ptr() == store.data_ptr() + 8 * shift
    snapshot = store.view(torch.int64).clone()
    torch.cuda.synchronize()
    ctx.set_contacts_device(view.data_ptr(), n, ld, keepalive=store)
    assert ctx.contacts_device() == (view.data_ptr(), n, ld)
    return store, snapshot


def assert_untouched(store, snapshot):
    """The adopted storage holds the bits it held when it was handed over (poison NaNs compare equal as integers)."""
    import torch
    if store.is_cuda:
        torch.cuda.synchronize()
    assert torch.equal(store.view(torch.int64), snapshot), "the adopted matrix was written to"


# ------------------------------------------------------------------------------------------------ readers of the matrix
_NEW = "test_gpu_adopted_ld.py::"
_SORTERS = [_NEW + "test_rank_matrix_per_call_sorters", _NEW + "test_rank_matrix_lds_sorter_in_a_fresh_process",
            _NEW + "test_rank_matrix_after_the_presort"]
_SHARD = "test_gpu_shard.py::test_adopted_matrix_under_a_shard"         # every first of stride 3, ld = n + 3
# callee of csrc/api.hip whose arguments begin `c->dC, c->ldc` (or the 2-D copy from c->dC) -> the tests that run it
# on a matrix with ld > n
READERS = {
    "launch_row_sums": [_NEW + "test_row_sums", _NEW + "test_row_sums_of_a_shard", _SHARD],
    "launch_compact": [_NEW + "test_compact"],
    "hipMemcpy2DAsync": [_NEW + "test_row_fetch", _NEW + "test_row_fetch_in_three_blocks"],
    "launch_build_w": [_NEW + "test_upgma", _NEW + "test_upgma_with_the_presort_beside_the_chain"],
    "launch_sort_rows": _SORTERS + [_SHARD],
    "launch_rank_rows_radix": [_NEW + "test_rank_matrix_per_call_sorters", _SHARD],
    "launch_similarity_row": [_NEW + "test_rank_matrix_per_call_sorters"],
    "launch_p2_select": [_NEW + "test_p2_literal_scores", _NEW + "test_workers_reports_equal_an_owned_copy"],
    "launch_plot_select": [_NEW + "test_plot_percentiles_and_downsample"],
    "launch_plot_downsample": [_NEW + "test_plot_percentiles_and_downsample"],
    "launch_hmm_obs": [_NEW + "test_hmm_observations"],
    "launch_louvain_graph": [_NEW + "test_louvain_graph"],
    # the four older tests
    "launch_group_sums": ["test_gpu_group_support.py::test_adopted_matrix_with_a_leading_dimension"],
    "launch_junction_sums": ["test_gpu_junctions.py::test_adopted_matrix_with_a_leading_dimension"],
    "launch_rebin": ["test_gpu_rebin.py::test_adopted_source_is_read_and_left_untouched"],
    # ICE rewrites the matrix in place: an adopted one is refused whole, so these never see a caller's ld
    "launch_ice_mask": ["test_gpu_ice.py::test_adopted_matrix_is_refused_and_untouched"],
    "launch_ice_rowdot": ["test_gpu_ice.py::test_adopted_matrix_is_refused_and_untouched"],
    "launch_ice_scale": ["test_gpu_ice.py::test_adopted_matrix_is_refused_and_untouched"],
    "launch_ice_apply": ["test_gpu_ice.py::test_adopted_matrix_is_refused_and_untouched"],
}

_CALL = re.compile(r"\b(\w+)\s*\(\s*c->dC\s*,\s*c->ldc\b")
_COPY2D = re.compile(r"\b(hipMemcpy2D\w*)\s*\([^;]*?\bc->dC\b[^;]*;")


def matrix_readers(source):
    """Names of the functions ``source`` (the text of csrc/api.hip) hands the contact matrix and its leading dimension."""
    return set(_CALL.findall(source)) | set(_COPY2D.findall(source))


def api_source():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "hic_genome_assembler_amd", "csrc", "api.hip")) as fh:
        return fh.read()
