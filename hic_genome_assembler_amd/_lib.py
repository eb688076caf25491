"""ctypes binding of libhicmi.so (include/hicmi.h) - the only way the Python host reaches the GPU.

There is deliberately no fallback: if the library has not been built, or no HIP device is
visible, the calls raise.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C hic_genome_assembler_amd/csrc``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HICMI_LIB") or os.path.join(_HERE, "libhicmi.so")     # HICMI_LIB: another build (A/B runs)
_lib = None

c_i64 = ctypes.c_int64
c_dbl = ctypes.c_double
_vp = ctypes.c_void_p
_M64 = (1 << 64) - 1

# name: (restype, argtypes) - one row per declaration in include/hicmi.h
SIGNATURES = {
    "hicmi_abi_version": (ctypes.c_int, []),
    "hicmi_last_error": (ctypes.c_char_p, []),
    "hicmi_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "hicmi_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "hicmi_destroy": (ctypes.c_int, [_vp]),
    "hicmi_stream": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "hicmi_synchronize": (ctypes.c_int, [_vp]),
    "hicmi_set_contacts_host": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_set_contacts_host_f32": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_set_contacts_device": (ctypes.c_int, [_vp, _vp, c_i64, c_i64]),
    "hicmi_contacts_device": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "hicmi_load_hicpro_matrix": (ctypes.c_int, [ctypes.c_char_p, _vp, c_i64, _vp, ctypes.c_int, ctypes.POINTER(c_i64)]),
    "hicmi_write_hicpro_matrix": (ctypes.c_int, [ctypes.c_char_p, _vp, c_i64, _vp, ctypes.c_int, ctypes.POINTER(c_i64)]),
    "hicmi_format_double": (ctypes.c_int, [c_dbl, ctypes.c_char_p, c_i64]),
    "hicmi_row_sums": (ctypes.c_int, [_vp, _vp, _vp]),
    "hicmi_set_row_shard": (ctypes.c_int, [_vp, c_i64, c_i64]),
    "hicmi_set_row_sums": (ctypes.c_int, [_vp, _vp, _vp]),
    "hicmi_compact": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_rebin": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_group_sums": (ctypes.c_int, [_vp, _vp, _vp, c_i64, c_i64, _vp, _vp]),
    "hicmi_junction_sums": (ctypes.c_int, [_vp, _vp, c_i64, _vp, c_i64, _vp]),
    "hicmi_get_contact_rows": (ctypes.c_int, [_vp, c_i64, c_i64, _vp]),
    "hicmi_ice_mask_rows": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_ice_balance": (ctypes.c_int, [_vp, _vp, c_i64, c_dbl, _vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_dbl)]),
    "hicmi_upgma": (ctypes.c_int, [_vp, _vp, _vp]),
    "hicmi_rank_matrix": (ctypes.c_int, [_vp, _vp]),
    "hicmi_presort_state": (ctypes.c_int, [_vp, _vp, _vp]),
    "hicmi_get_rank_rows": (ctypes.c_int, [_vp, c_i64, c_i64, ctypes.c_int, _vp]),
    "hicmi_get_similarity_row": (ctypes.c_int, [_vp, c_i64, _vp]),
    "hicmi_cut_scan": (ctypes.c_int, [_vp, c_i64, c_i64, c_dbl, _vp, _vp]),
    "hicmi_filter_scan": (ctypes.c_int, [_vp, c_i64, c_i64, c_i64, c_i64, c_dbl, _vp, _vp]),
    "hicmi_first_pass_cuts": (ctypes.c_int, [_vp, c_i64, c_i64, c_dbl, _vp, c_i64, _vp, _vp, c_i64, _vp]),
    "hicmi_filter_cuts": (ctypes.c_int, [_vp, _vp, c_i64, c_dbl, _vp, c_i64, _vp, _vp]),
    "hicmi_first_pass_cuts_multi": (ctypes.c_int, [_vp, c_i64, _vp, _vp, c_dbl, _vp, c_i64, _vp, _vp, c_i64, _vp]),
    "hicmi_filter_cuts_multi": (ctypes.c_int, [_vp, c_i64, _vp, _vp, _vp, _vp, c_i64, _vp, _vp]),
    "hicmi_hypergeom_decide": (ctypes.c_int, [c_i64, c_i64, c_i64, c_i64, c_dbl]),
    "hicmi_hypergeom_sf": (c_dbl, [c_i64, c_i64, c_i64, c_i64]),
    "hicmi_selftest_division": (ctypes.c_int, [_vp, ctypes.c_uint64, c_i64, ctypes.POINTER(ctypes.c_uint64)]),
    "hicmi_label_linkage": (ctypes.c_int, [_vp, c_i64, _vp]),
    "hicmi_leaf_order": (ctypes.c_int, [_vp, c_i64, _vp]),
    "hicmi_get_raw_merges": (ctypes.c_int, [_vp, _vp]),
    "hicmi_nnchain_stats": (ctypes.c_int, [_vp, _vp]),
    "hicmi_p2_select": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_p2_total": (ctypes.c_int, [_vp, ctypes.POINTER(c_dbl)]),
    "hicmi_p2_score": (ctypes.c_int, [_vp, _vp, c_i64, c_i64, c_dbl, _vp]),
    "hicmi_p2_score_exact": (ctypes.c_int, [_vp, _vp, c_i64, c_i64, c_dbl, _vp]),
    "hicmi_p2_layout": (ctypes.c_int, [_vp, _vp, _vp, c_i64]),
    "hicmi_p2_set_arrangement": (ctypes.c_int, [_vp, _vp, _vp, c_i64]),
    "hicmi_p2_arrangement_total": (ctypes.c_int, [_vp, ctypes.POINTER(c_dbl)]),
    "hicmi_p2_arrangement_score": (ctypes.c_int, [_vp, c_dbl, ctypes.POINTER(c_dbl)]),
    "hicmi_p2_score_insertions": (ctypes.c_int, [_vp, ctypes.c_int32, c_dbl, _vp]),
    "hicmi_p2_window_tables": (ctypes.c_int, [_vp, c_i64, _vp, c_i64, _vp, c_i64]),
    "hicmi_p2_score_window": (ctypes.c_int, [_vp, c_i64, c_i64, _vp]),
    "hicmi_p2_decide_window": (ctypes.c_int, [_vp, c_i64, c_i64, c_dbl, c_dbl, c_dbl, ctypes.POINTER(c_i64),
                                              ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl)]),
    "hicmi_p2_window_shortlist": (ctypes.c_int, [_vp, c_i64, c_i64, c_i64, c_dbl, c_dbl, c_dbl, c_i64, _vp, _vp, _vp]),
    "hicmi_p2_decide_insertion": (ctypes.c_int, [_vp, _vp, _vp, c_i64, ctypes.c_int32, ctypes.c_int32,
                                                 ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_int32),
                                                 ctypes.POINTER(c_dbl)]),
    "hicmi_p2_insert_all": (ctypes.c_int, [_vp, _vp, _vp, c_i64, _vp, c_i64, ctypes.POINTER(c_dbl)]),
    "hicmi_scan_valid_pairs": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, _vp, c_i64, ctypes.c_int,
                                              ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), ctypes.POINTER(_vp)]),
    "hicmi_scan_fetch": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "hicmi_parse_valid_pairs": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, ctypes.c_int, c_i64, c_i64,
                                               _vp, _vp, _vp, _vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), _vp]),
    "hicmi_map_begin": (ctypes.c_int, [_vp, _vp, c_i64, c_i64]),
    "hicmi_map_add_pairs": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, c_i64]),
    "hicmi_map_finish": (ctypes.c_int, [_vp, ctypes.POINTER(c_i64)]),
    "hicmi_build_maps": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, c_i64, _vp, _vp, ctypes.c_int, _vp]),
    "hicmi_map_begin_lifted": (ctypes.c_int, [_vp, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, c_i64]),
    "hicmi_pair_stats": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, c_i64, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, _vp, _vp, _vp, _vp]),
    "hicmi_lift_maps": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, _vp, _vp, _vp, _vp, c_i64, c_i64, _vp, _vp,
                                       ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "hicmi_span_begin": (ctypes.c_int, [_vp, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, c_i64, c_i64, _vp, ctypes.POINTER(c_i64)]),
    "hicmi_span_add_pairs": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, c_i64]),
    "hicmi_span_finish": (ctypes.c_int, [_vp, c_i64, _vp, c_i64, _vp, _vp, _vp]),
    "hicmi_span_file": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, _vp, _vp, _vp, _vp, c_i64, c_i64, c_i64,
                                       c_i64, _vp, c_i64, _vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(c_i64)]),
    "hicmi_ends_begin": (ctypes.c_int, [_vp, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, c_i64, c_i64, _vp, ctypes.POINTER(c_i64)]),
    "hicmi_ends_add_pairs": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, c_i64]),
    "hicmi_ends_finish": (ctypes.c_int, [_vp, _vp, _vp]),
    "hicmi_ends_file": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, _vp, _vp, _vp, _vp, c_i64, c_i64, c_i64,
                                       _vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.POINTER(c_i64)]),
    "hicmi_anchor_begin": (ctypes.c_int, [_vp, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, _vp, c_i64, _vp, ctypes.POINTER(c_i64)]),
    "hicmi_anchor_add_pairs": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, c_i64]),
    "hicmi_anchor_finish": (ctypes.c_int, [_vp, _vp, _vp]),
    "hicmi_anchor_file": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, _vp, _vp, _vp, _vp, c_i64, _vp, c_i64,
                                         _vp, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.POINTER(c_i64)]),
    "hicmi_pairs_begin": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_pairs_add": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, c_i64]),
    "hicmi_pairs_file": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, _vp, ctypes.c_int, _vp]),
    "hicmi_pairs_info": (ctypes.c_int, [_vp, ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_uint64), _vp]),
    "hicmi_pairs_fetch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "hicmi_pairs_drop": (ctypes.c_int, [_vp]),
    "hicmi_ends_resident": (ctypes.c_int, [_vp, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, c_i64, c_i64, _vp, _vp, _vp, ctypes.POINTER(c_i64)]),
    "hicmi_anchor_resident": (ctypes.c_int, [_vp, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, _vp, c_i64, _vp, _vp, _vp,
                                             ctypes.POINTER(c_i64)]),
    "hicmi_seats_resident": (ctypes.c_int, [_vp, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, c_i64, _vp, _vp, _vp,
                                            ctypes.POINTER(c_i64)]),
    "hicmi_links_resident": (ctypes.c_int, [_vp, _vp, c_i64, c_i64, ctypes.POINTER(c_i64), _vp]),
    "hicmi_links_fetch": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "hicmi_links_info": (ctypes.c_int, [_vp, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), ctypes.POINTER(ctypes.c_double)]),
    "hicmi_links_lifted": (ctypes.c_int, [_vp, _vp, c_i64, _vp, _vp, _vp, _vp, c_i64, c_i64, ctypes.POINTER(c_i64), _vp]),
    "hicmi_split_pairs": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, c_i64, _vp, c_i64, _vp, _vp, c_i64, _vp, _vp, _vp, _vp, _vp]),
    "hicmi_split_maps": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, _vp, _vp, c_i64, c_i64, _vp, _vp,
                                        ctypes.c_int, _vp, _vp]),
    "hicmi_split_valid_pairs": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, _vp, c_i64, _vp, _vp, _vp, c_i64,
                                               ctypes.c_char_p, _vp, ctypes.c_int, _vp]),
    "hicmi_plot_percentiles": (ctypes.c_int, [_vp, ctypes.c_int, _vp, c_i64, _vp, c_i64, _vp]),
    "hicmi_plot_downsample": (ctypes.c_int, [_vp, ctypes.c_int, _vp, c_i64, c_i64, _vp]),
    "hicmi_p2_insert_all_multi": (ctypes.c_int, [c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hicmi_p2_start_all": (ctypes.c_int, [c_i64] + [_vp] * 16),
    "hicmi_p2_scan_arranged": (ctypes.c_int, [_vp, _vp, _vp, c_i64, c_i64, _vp, c_i64, _vp, c_i64, ctypes.POINTER(c_dbl),
                                              ctypes.POINTER(c_dbl), ctypes.POINTER(c_i64)]),
    "hicmi_p2_support": (ctypes.c_int, [_vp, _vp, _vp, c_i64, c_dbl, _vp, _vp]),
    "hicmi_p2_support_multi": (ctypes.c_int, [c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hicmi_p2_breaks": (ctypes.c_int, [_vp, _vp, _vp, c_i64, c_dbl, c_i64, _vp, _vp]),
    "hicmi_p2_breaks_multi": (ctypes.c_int, [c_i64, _vp, _vp, _vp, _vp, _vp, c_i64, _vp, _vp]),
    "hicmi_p2_inversions": (ctypes.c_int, [_vp, _vp, _vp, c_i64, c_dbl, c_i64, _vp, _vp]),
    "hicmi_p2_inversions_multi": (ctypes.c_int, [c_i64, _vp, _vp, _vp, _vp, _vp, c_i64, _vp, _vp]),
    "hicmi_p2_scan_pass": (ctypes.c_int, [_vp, _vp, _vp, c_i64, c_i64, c_dbl, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl),
                                          ctypes.POINTER(ctypes.c_int32)]),
    "hicmi_p2_scan_all": (ctypes.c_int, [_vp, _vp, _vp, c_i64, c_i64, c_dbl, ctypes.POINTER(c_dbl), ctypes.POINTER(c_dbl),
                          ctypes.POINTER(c_i64)]),
    "hicmi_hmm_load_obs": (ctypes.c_int, [_vp, _vp, c_i64, c_i64, c_i64]),
    "hicmi_hmm_set_obs": (ctypes.c_int, [_vp, _vp, c_i64, c_i64]),
    "hicmi_hmm_set_width": (ctypes.c_int, [_vp, c_i64]),
    "hicmi_hmm_get_obs": (ctypes.c_int, [_vp, c_i64, c_i64, _vp]),
    "hicmi_hmm_dist2": (ctypes.c_int, [_vp, _vp, c_i64, _vp]),
    "hicmi_hmm_col_stats": (ctypes.c_int, [_vp, _vp, _vp]),
    "hicmi_hmm_kmeans": (ctypes.c_int, [_vp, _vp, c_i64, c_dbl, _vp, _vp, ctypes.POINTER(c_dbl), ctypes.POINTER(c_i64)]),
    "hicmi_hmm_fit": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, c_i64, c_dbl, _vp, ctypes.POINTER(c_i64)]),
    "hicmi_hmm_decode": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "hicmi_hmm_load_obs_slot": (ctypes.c_int, [_vp, c_i64, _vp, c_i64, c_i64, c_i64]),
    "hicmi_hmm_use_obs": (ctypes.c_int, [_vp, c_i64]),
    "hicmi_hmm_dist2_multi": (ctypes.c_int, [_vp, c_i64, _vp, _vp, _vp, _vp, _vp]),
    "hicmi_hmm_kmeans_multi": (ctypes.c_int, [_vp, c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hicmi_louvain_graph": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_louvain_set_graph": (ctypes.c_int, [_vp, _vp, c_i64]),
    "hicmi_louvain_get_graph": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "hicmi_louvain_level0": (ctypes.c_int, [_vp, c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hicmi_louvain_induced": (ctypes.c_int, [_vp, _vp, c_i64, c_i64, _vp]),
    "hicmi_louvain_modularity": (ctypes.c_int, [_vp, _vp, c_i64, c_i64, _vp]),
    "hicmi_timing_reset": (ctypes.c_int, [_vp]),
    "hicmi_timing_enable": (ctypes.c_int, [_vp, ctypes.c_int]),
    "hicmi_timing_get": (ctypes.c_int, [_vp, ctypes.c_char_p, c_i64, _vp, _vp, _vp, c_i64, ctypes.POINTER(c_i64)]),
}


class HicmiError(RuntimeError):
    pass


def load():
    """Load libhicmi.so and attach signatures.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HicmiError("libhicmi.so is not built (%s): run `make -C %s` - this package has no CPU fallback"
                         % (LIB_PATH, os.path.join(_HERE, "csrc")))
    try:
        # PyTorch-ROCm bundles its own libamdhip64; if a second copy (the /opt/rocm one libhicmi links
        # against) initialises first, torch later reports "no ROCm-capable device".  Loading torch
        # first makes both share one HIP runtime.  torch is plumbing only (device buffers, RCCL).
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.hicmi_abi_version() != 1:
        raise HicmiError("libhicmi ABI version mismatch")
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise HicmiError("libhicmi error %d: %s" % (rc, load().hicmi_last_error().decode("utf-8", "replace")))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def load_hicpro_matrix(path, bin_ids, threads: int = 0):
    """Dense fp64 matrix from a HiC-Pro triplet file, parsed by libhicmi's multi-threaded host loader."""
    ids = np.ascontiguousarray(bin_ids, dtype=np.int64)
    n = len(ids)
    out = np.empty((n, n), dtype=np.float64)
    edges = c_i64()
    _check(load().hicmi_load_hicpro_matrix(os.fsencode(path), _ptr(ids), n, _ptr(out), int(threads), ctypes.byref(edges)))
    return out, edges.value


def write_hicpro_matrix(path, mat, bin_ids, threads: int = 0) -> int:
    """HiC-Pro triplet file of a dense symmetric fp64 matrix, written by libhicmi's multi-threaded host formatter
    (hicmi_write_hicpro_matrix); returns the number of lines."""
    mat = np.ascontiguousarray(mat, dtype=np.float64)
    ids = np.ascontiguousarray(bin_ids, dtype=np.int64)
    if mat.ndim != 2 or mat.shape[0] != mat.shape[1] or mat.shape[0] != len(ids):
        raise ValueError("mat must be n x n with one bin ID per row")
    entries = c_i64()
    _check(load().hicmi_write_hicpro_matrix(os.fsencode(path), _ptr(mat), len(ids), _ptr(ids), int(threads), ctypes.byref(entries)))
    return entries.value


def format_double(v) -> str:
    """repr(float(v)) as libhicmi's writer formats it (hicmi_format_double)."""
    buf = ctypes.create_string_buffer(64)
    _check(load().hicmi_format_double(float(v), buf, 64))
    return buf.value.decode("ascii")


def scan_valid_pairs(path, names, pairs, threads: int = 0):
    """Lines of a HiC-Pro allValidPairs file that name one of the ordered scaffold pairs ``pairs`` (indices
    into ``names``): returns (pair index, pos1, pos2) arrays in file order and the number of lines read."""
    blob, off = _name_blob(names)
    pa = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
    pb = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
    n_hits, n_lines, handle = c_i64(), c_i64(), _vp()
    _check(load().hicmi_scan_valid_pairs(os.fsencode(path), blob, _ptr(off), len(off) - 1, _ptr(pa), _ptr(pb), len(pa), int(threads),
                                         ctypes.byref(n_hits), ctypes.byref(n_lines), ctypes.byref(handle)))
    idx = np.empty(n_hits.value, np.int32)
    p1 = np.empty(n_hits.value, np.int64)
    p2 = np.empty(n_hits.value, np.int64)
    _check(load().hicmi_scan_fetch(handle, _ptr(idx), _ptr(p1), _ptr(p2)))
    return idx, p1, p2, n_lines.value


def _name_blob(names):
    """(concatenated UTF-8 names, int64 offsets) as the valid-pair readers take them."""
    enc = [n.encode("utf-8") for n in names]
    off = np.zeros(len(enc) + 1, np.int64)
    if enc:
        off[1:] = np.cumsum([len(e) for e in enc])
    return b"".join(enc), off


def _names_and_sizes(names, sizes, and_ok=True, and_what=""):
    """(name blob, int64 offsets, int64 sizes) of the scaffolds of a pair file, one size per name.  ``and_ok`` and
    ``and_what``: a second condition of the caller's and the words that name it in the same refusal."""
    blob, off = _name_blob(names)
    size = np.ascontiguousarray(sizes, dtype=np.int64)
    if size.shape != (len(names),) or not and_ok:
        raise ValueError("one size per scaffold name" + and_what)
    return blob, off, size


def _pair_arrays(scaf_a, pos_a, scaf_b, pos_b):
    """A chunk of pairs as the library takes it: (scaf_a int32, pos_a int64, scaf_b int32, pos_b int64), contiguous
    vectors of one length."""
    sa, sb = np.ascontiguousarray(scaf_a, dtype=np.int32), np.ascontiguousarray(scaf_b, dtype=np.int32)
    pa, pb = np.ascontiguousarray(pos_a, dtype=np.int64), np.ascontiguousarray(pos_b, dtype=np.int64)
    if not (sa.ndim == 1 and sa.shape == sb.shape == pa.shape == pb.shape):
        raise ValueError("the four arrays must be vectors of one length")
    return sa, pa, sb, pb


def parse_valid_pairs(path, names, sizes, first_byte: int = 0, max_pairs=None, threads: int = 0):
    """Up to ``max_pairs`` read pairs of a HiC-Pro allValidPairs file from ``first_byte`` on (hicmi_parse_valid_pairs,
    DESIGN.md 9l): (scaffold a, position a, scaffold b, position b) in file order - indices into ``names``, 1-based
    positions - then next_byte (the file size when the file is done) and (lines, used, unknown_scaffold, out_of_range).
    ``max_pairs=None``: as many as the rest of the file can hold."""
    blob, off, size = _names_and_sizes(names, sizes)
    if max_pairs is None:
        try:
            max_pairs = max(1, (os.path.getsize(path) - int(first_byte)) // 12 + 1)     # a six-column line has 12 bytes or more
        except OSError:
            max_pairs = 1                                                               # the library reports the file
    max_pairs = int(max_pairs)
    sa, sb = np.empty(max(max_pairs, 0), np.int32), np.empty(max(max_pairs, 0), np.int32)
    pa, pb = np.empty(max(max_pairs, 0), np.int64), np.empty(max(max_pairs, 0), np.int64)
    n, nxt, stats = c_i64(), c_i64(), np.zeros(4, np.int64)
    _check(load().hicmi_parse_valid_pairs(os.fsencode(path), blob, _ptr(off), len(names), _ptr(size), int(threads), int(first_byte),
                                          max_pairs, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb), ctypes.byref(n), ctypes.byref(nxt),
                                          _ptr(stats)))
    k = n.value
    return sa[:k], pa[:k], sb[:k], pb[:k], nxt.value, tuple(int(v) for v in stats)


def build_maps(path, names, sizes, resolutions, ctxs, threads: int = 0):
    """One pass over a HiC-Pro allValidPairs file for the raw maps at every resolution of ``resolutions``, ``ctxs[k]``
    receiving the map at ``resolutions[k]`` (hicmi_build_maps); the contexts are distinct and on one GPU.
    Returns (lines, used, unknown_scaffold, out_of_range, chunks)."""
    res = np.ascontiguousarray(resolutions, dtype=np.int64)
    blob, off, size = _names_and_sizes(names, sizes, res.ndim == 1 and len(res) == len(ctxs) and len(ctxs) > 0,
                                       " and one context per resolution")
    handles = (_vp * len(ctxs))(*[c._h for c in ctxs])
    stats = np.zeros(5, np.int64)
    _check(load().hicmi_build_maps(os.fsencode(path), blob, _ptr(off), len(names), _ptr(size), len(res), _ptr(res), handles,
                                   int(threads), _ptr(stats)))
    for c in ctxs:
        c.n = c.contacts_device()[1]
        c._keepalive = None
        c._matrix_replaced()
    return tuple(int(v) for v in stats)


def _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes):
    """The lift tables of DESIGN.md 9m as the library takes them: (scaffold sizes, lift_seq int32, lift_off int64,
    lift_rev uint8, sequence sizes), one entry per scaffold and one size per sequence."""
    size = np.ascontiguousarray(sizes, dtype=np.int64)
    seq = np.ascontiguousarray(lift_seq, dtype=np.int32)
    off = np.ascontiguousarray(lift_off, dtype=np.int64)
    rev = np.ascontiguousarray(lift_rev, dtype=np.uint8)
    seq_size = np.ascontiguousarray(seq_sizes, dtype=np.int64)
    if size.ndim != 1 or not (seq.shape == off.shape == rev.shape == size.shape) or seq_size.ndim != 1:
        raise ValueError("one lift_seq, lift_off and lift_rev per scaffold size, and a vector of sequence sizes")
    return size, seq, off, rev, seq_size


def new_pair_stats(n_seq):
    """Zeroed (decay[256], seq_cis[n_seq], seq_trans[n_seq], unlifted[1]) for Context.pair_stats and lift_maps to add to."""
    return (np.zeros(256, np.uint64), np.zeros(int(n_seq), np.uint64), np.zeros(int(n_seq), np.uint64), np.zeros(1, np.uint64))


def _pair_stats_into(into, n_seq):
    if into is None:
        return new_pair_stats(n_seq)
    decay, cis, trans, unlifted = into
    for a, shape in ((decay, (256,)), (cis, (n_seq,)), (trans, (n_seq,)), (unlifted, (1,))):
        if a.dtype != np.uint64 or a.shape != shape or not a.flags.c_contiguous or not a.flags.writeable:
            raise ValueError("into must be what new_pair_stats(n_seq) returns")
    return into


def lift_maps(path, names, sizes, lift_seq, lift_off, lift_rev, seq_sizes, resolutions, ctxs, threads: int = 0, into=None):
    """build_maps in the coordinates of an assembly (hicmi_lift_maps): one pass over the pair file for the
    lifted maps at every resolution - ``ctxs[k]`` receives the one at ``resolutions[k]`` - and the statistics of the
    pairs, added to ``into`` (new_pair_stats; None: fresh ones).  Returns ((lines, used, unknown_scaffold, out_of_range,
    chunks), (decay, seq_cis, seq_trans, unlifted))."""
    size, seq, loff, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
    res = np.ascontiguousarray(resolutions, dtype=np.int64)
    blob, off, size = _names_and_sizes(names, size, res.ndim == 1 and len(res) == len(ctxs) and len(ctxs) > 0,
                                       " and one context per resolution")
    out = _pair_stats_into(into, len(seq_size))
    handles = (_vp * len(ctxs))(*[c._h for c in ctxs])
    stats = np.zeros(5, np.int64)
    _check(load().hicmi_lift_maps(os.fsencode(path), blob, _ptr(off), len(names), _ptr(size), _ptr(seq), _ptr(loff), _ptr(rev),
                                  _ptr(seq_size), len(seq_size), len(res), _ptr(res), handles, int(threads), _ptr(stats),
                                  _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _ptr(out[3])))
    for c in ctxs:
        c.n = c.contacts_device()[1]
        c._keepalive = None
        c._matrix_replaced()
    return tuple(int(v) for v in stats), out


def _span_records(recs):
    """The records (lo, hi, q0, q1) of a span call as a contiguous int64 array of shape (n_rec, 4)."""
    rec = np.ascontiguousarray(recs, dtype=np.int64).reshape(-1, 4)
    return rec, np.zeros((len(rec), 4), np.int64)


def span_cell_count(sizes, lift_seq, step) -> int:
    """Cells of a span build: ceil(L / step) for every placed scaffold of size L > 0."""
    size = np.asarray(sizes, dtype=np.int64)
    placed = size[(np.asarray(lift_seq) >= 0) & (size > 0)]
    step = int(step)
    return int((placed // step + (placed % step != 0)).sum()) if step >= 1 else 0


def span_file(path, names, sizes, lift_seq, lift_off, lift_rev, seq_sizes, step, max_span, flank, recs, ctx, threads: int = 0,
              want_depth: bool = True):
    """Spanning depth of an assembly over a HiC-Pro allValidPairs file in one pass (hicmi_span_file) on the
    device of ``ctx``, whose matrix and open map build stay as they are.  ``recs``: records (lo, hi, q0, q1) of slots.
    Returns ((lines, used, unknown_scaffold, out_of_range, chunks), cell_first int64[S], picks int64[n_rec, 4] = (slot, D,
    Lsum, Rsum), counters uint64[5] = (marked, one_cell, beyond_max_span, trans, unlifted), depth uint64[n_cells] or None)."""
    size, seq, loff, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
    blob, off, size = _names_and_sizes(names, size)
    rec, picks = _span_records(recs)
    stats, counters = np.zeros(5, np.int64), np.zeros(5, np.uint64)
    cell_first, n_cells = np.zeros(len(size), np.int64), c_i64()
    depth = np.zeros(max(span_cell_count(size, seq, step), 1), np.uint64) if want_depth else None
    _check(load().hicmi_span_file(os.fsencode(path), blob, _ptr(off), len(names), _ptr(size), _ptr(seq), _ptr(loff), _ptr(rev),
                                  _ptr(seq_size), len(seq_size), int(step), int(max_span), int(flank), _ptr(rec), len(rec), ctx._h,
                                  int(threads), _ptr(stats), _ptr(picks), _ptr(counters), _ptr(depth), _ptr(cell_first),
                                  ctypes.byref(n_cells)))
    return tuple(int(v) for v in stats), cell_first, picks, counters, None if depth is None else depth[:n_cells.value]


ENDS_MAX_TABLE = 1 << 27


def ends_placed_count(sizes, lift_seq) -> int:
    """Placed scaffolds of an ends build: those of a sequence and of size > 0."""
    size = np.asarray(sizes, dtype=np.int64)
    return int(((np.asarray(lift_seq) >= 0) & (size > 0)).sum())


def _ends_table(n_placed, reach):
    """A zeroed table uint64[P, reach, 4] for the library to fill; one counter where it will refuse the build."""
    reach = int(reach)
    ok = 1 <= reach <= 64 and 1 <= n_placed and n_placed * reach * 4 <= ENDS_MAX_TABLE
    return np.zeros((n_placed, reach, 4) if ok else (1, 1, 4), np.uint64)


def ends_file(path, names, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window, reach, ctx, threads: int = 0):
    """End support of an assembly over a HiC-Pro allValidPairs file in one pass (hicmi_ends_file) on the
    device of ``ctx``, whose matrix, open map build and open span build stay as they are.  Returns ((lines, used,
    unknown_scaffold, out_of_range, chunks), rank int32[S], table uint64[P, reach, 4], counters uint64[6] = (linked, middle,
    same, too_far, trans, unlifted))."""
    size, seq, loff, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
    blob, off, size = _names_and_sizes(names, size)
    stats, counters = np.zeros(5, np.int64), np.zeros(6, np.uint64)
    rank, n_placed = np.zeros(len(size), np.int32), c_i64()
    table = _ends_table(ends_placed_count(size, seq), reach)
    _check(load().hicmi_ends_file(os.fsencode(path), blob, _ptr(off), len(names), _ptr(size), _ptr(seq), _ptr(loff), _ptr(rev),
                                  _ptr(seq_size), len(seq_size), int(window), int(reach), ctx._h, int(threads), _ptr(stats),
                                  _ptr(table), _ptr(counters), _ptr(rank), ctypes.byref(n_placed)))
    return tuple(int(v) for v in stats), rank, table, counters


ANCHOR_MAX_TABLE = 1 << 27
SEATS_MAX_TABLE = 1 << 27
# the end-link graph: scaffolds of a call, slots of its table, and the sizes of the combining kernel's slice
# and table in LDS (csrc/hicmi_internal.h), which the tests place their edge cases at
LINKS_MAX_SCAF, LINKS_MIN_SLOTS, LINKS_MAX_SLOTS = 1 << 30, 1024, 1 << 31
LINKS_SLICE, LINKS_SLOTS = 8192, 2048
LINKS_COLUMNS = ("left_left", "left_right", "right_left", "right_right", "other")


def links_capacity(n_kept, n_scaf):
    """Slots of the find-or-insert table of a ``links_resident`` call: the smallest power of two that is at least 1,024 and
    at least twice min(n_kept, 5 n_scaf (n_scaf - 1) / 2)."""
    most = min(int(n_kept), 5 * int(n_scaf) * (int(n_scaf) - 1) // 2) if n_kept > 0 and n_scaf > 1 else 0
    cap = LINKS_MIN_SLOTS
    while cap < 2 * most:
        cap *= 2
    return cap


def anchor_blocks(sizes, lift_seq, n_seq, target=None):
    """(first int64[S], n_table) of an anchor build: the candidates - the dropped scaffolds of size > 0, in
    rank mode those with ``target`` >= 0 - in index order, each with a block of ``n_seq`` counters or, in rank mode, of four
    per placed scaffold of size > 0 of its target sequence; -1 for a scaffold that is no candidate.  n_table is -1 for
    targets the library will refuse."""
    size, seq = np.asarray(sizes, dtype=np.int64), np.asarray(lift_seq, dtype=np.int64)
    candidate = (seq < 0) & (size > 0)
    if target is None:
        block = np.full(len(size), int(n_seq), np.int64)
    else:
        tgt = np.asarray(target, dtype=np.int64)
        if tgt.shape != size.shape or ((tgt < -1) | (tgt >= int(n_seq))).any() or (~candidate & (tgt >= 0)).any():
            return np.full(len(size), -1, np.int64), -1
        placed = np.bincount(seq[(seq >= 0) & (seq < int(n_seq)) & (size > 0)], minlength=int(n_seq))
        candidate = tgt >= 0
        block = 4 * placed[np.where(candidate, tgt, 0)]
    ends = np.cumsum(np.where(candidate, block, 0))
    first = np.where(candidate, ends - block, -1).astype(np.int64)
    return first, int(ends[-1]) if len(ends) else 0


def _anchor_table(n_table):
    """A zeroed table for the library to fill; one counter where it will refuse the build."""
    return np.zeros(n_table if 1 <= n_table <= ANCHOR_MAX_TABLE else 1, np.uint64)


def seats_blocks(sizes, lift_seq, n_seq):
    """(first int64[S], n_table) of a seat-support call: the placed scaffolds of size > 0 in index order, each
    with a block of ``n_seq`` counters and four per placed scaffold of size > 0 of its own sequence; -1 for a dropped or empty
    scaffold."""
    size, seq = np.asarray(sizes, dtype=np.int64), np.asarray(lift_seq, dtype=np.int64)
    placed = (seq >= 0) & (seq < int(n_seq)) & (size > 0)
    members = np.bincount(seq[placed], minlength=int(n_seq)).astype(np.int64)
    block = np.where(placed, int(n_seq) + 4 * members[np.where(placed, seq, 0)], 0)
    ends = np.cumsum(block)
    return np.where(placed, ends - block, -1).astype(np.int64), int(ends[-1]) if len(ends) else 0


def _anchor_target(target, n_scaf):
    if target is None:
        return None
    tgt = np.ascontiguousarray(target, dtype=np.int32)
    if tgt.shape != (n_scaf,):
        raise ValueError("one target per scaffold size")
    return tgt


def anchor_file(path, names, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window, ctx, threads: int = 0):
    """Anchoring of the scaffolds an assembly leaves out over a HiC-Pro allValidPairs file in one pass (hicmi_anchor_file,
    DESIGN.md 9q) on the device of ``ctx``, whose matrix, open map build, open span build and open ends build stay as they
    are.  ``target`` None: sequence mode, else the target sequence of every scaffold (-1: none).  Returns ((lines, used,
    unknown_scaffold, out_of_range, chunks), first int64[S], table uint64[n_table], counters uint64[6] = (anchored, middle,
    elsewhere, skipped, unplaced, placed))."""
    size, seq, loff, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
    blob, off, size = _names_and_sizes(names, size)
    tgt =_anchor_target(target, len(size))
    stats, counters = np.zeros(5, np.int64), np.zeros(6, np.uint64)
    first, n_table = np.zeros(len(size), np.int64), c_i64()
    table = _anchor_table(anchor_blocks(size, seq, len(seq_size), tgt)[1])
    _check(load().hicmi_anchor_file(os.fsencode(path), blob, _ptr(off), len(names), _ptr(size), _ptr(seq), _ptr(loff), _ptr(rev),
                                    _ptr(seq_size), len(seq_size), _ptr(tgt), int(window), ctx._h, int(threads), _ptr(stats),
                                    _ptr(table), _ptr(counters), _ptr(first), ctypes.byref(n_table)))
    return tuple(int(v) for v in stats), first, table, counters


def pairs_file(path, names, sizes, ctx, threads: int = 0):
    """Load a HiC-Pro allValidPairs file into the resident pair store of ``ctx`` in one pass (hicmi_pairs_file, DESIGN.md
    9r): the pairs on two scaffolds stay on the device, the others are counted per scaffold.  The matrix and every open
    build of ``ctx`` stay as they are.  Returns (lines, used, unknown_scaffold, out_of_range, chunks)."""
    blob, off, size = _names_and_sizes(names, sizes)
    stats = np.zeros(5, np.int64)
    _check(load().hicmi_pairs_file(os.fsencode(path), blob, _ptr(off), len(names), _ptr(size), ctx._h, int(threads), _ptr(stats)))
    ctx._pairs_scaffolds = len(size)
    return tuple(int(v) for v in stats)


def _split_tables(sizes, piece_first, piece_start):
    """The piece tables of DESIGN.md 9o as the library takes them: (scaffold sizes, piece_first int32[S + 1], piece_start
    int64[n_piece])."""
    size = np.ascontiguousarray(sizes, dtype=np.int64)
    first = np.ascontiguousarray(piece_first, dtype=np.int32)
    start = np.ascontiguousarray(piece_start, dtype=np.int64)
    if size.ndim != 1 or first.shape != (len(size) + 1,) or start.ndim != 1:
        raise ValueError("one piece_first per scaffold size and one more, and a vector of piece starts")
    return size, first, start


def new_split_counters(n_piece):
    """Zeroed counters uint64[4, n_piece] = (within, sibling, other, mark) for Context.split_pairs and split_maps to add to."""
    return np.zeros((4, int(n_piece)), np.uint64)


def _split_counters_into(into, n_piece):
    if into is None:
        return new_split_counters(n_piece)
    if into.dtype != np.uint64 or into.shape != (4, n_piece) or not into.flags.c_contiguous or not into.flags.writeable:
        raise ValueError("into must be what new_split_counters(n_piece) returns")
    return into


def split_spanning(piece_first, counters):
    """``spanning`` of every piece from the mark row of the counters: the prefix sum of the marks inside each scaffold
    (uint64, wrapping), which is the number of pairs of the scaffold with one end at or before the piece's last base and one
    after it; 0 at the last piece of a scaffold."""
    first = np.asarray(piece_first, dtype=np.int64)
    mark = np.asarray(counters, dtype=np.uint64).reshape(4, -1)[3]
    total = np.cumsum(mark, dtype=np.uint64)
    before = np.concatenate([np.zeros(1, np.uint64), total])[first[:-1]]
    return total - np.repeat(before, np.diff(first))


def split_maps(path, names, sizes, piece_first, piece_start, resolutions, ctxs, threads: int = 0, into=None):
    """build_maps on the pieces the scaffolds are cut into (hicmi_split_maps): one pass over the pair file,
    every chunk moved from the scaffolds to the pieces on the device and counted into the map of every resolution -
    ``ctxs[k]`` receives the one at ``resolutions[k]``, cut from the pieces - and the counters of the pieces, added to
    ``into`` (new_split_counters; None: fresh ones).  No resolution: the counters alone, on the device of ``ctxs[0]``,
    which is left as it is.  Returns ((lines, used, unknown_scaffold, out_of_range, chunks), counters)."""
    size, first, start = _split_tables(sizes, piece_first, piece_start)
    res = np.ascontiguousarray(resolutions, dtype=np.int64).reshape(-1)
    blob, off, size = _names_and_sizes(names, size, len(ctxs) > 0 and len(ctxs) == max(len(res), 1),
                                       " and one context per resolution (one context when there is no resolution)")
    out =_split_counters_into(into, len(start))
    handles = (_vp * len(ctxs))(*[c._h for c in ctxs])
    stats = np.zeros(5, np.int64)
    _check(load().hicmi_split_maps(os.fsencode(path), blob, _ptr(off), len(names), _ptr(size), _ptr(first), _ptr(start), len(start),
                                   len(res), _ptr(res), handles, int(threads), _ptr(stats), _ptr(out)))
    if len(res):
        for c in ctxs:
            c.n = c.contacts_device()[1]
            c._keepalive = None
            c._matrix_replaced()
    return tuple(int(v) for v in stats), out


def split_valid_pairs(path_in, path_out, names, sizes, piece_first, piece_start, piece_names, threads: int = 0):
    """``path_in`` written again as ``path_out`` with both ends of every kept line moved to the pieces
    (hicmi_split_valid_pairs; host code).  Returns (lines, used, unknown_scaffold, out_of_range)."""
    piece_blob, piece_off = _name_blob(piece_names)
    size, first, start = _split_tables(sizes, piece_first, piece_start)
    blob, off, size = _names_and_sizes(names, size, len(piece_names) == len(start), " and one name per piece")
    stats = np.zeros(4, np.int64)
    _check(load().hicmi_split_valid_pairs(os.fsencode(path_in), os.fsencode(path_out), blob, _ptr(off), len(names), _ptr(size),
                                          _ptr(first), _ptr(start), len(start), piece_blob, _ptr(piece_off), int(threads),
                                          _ptr(stats)))
    return tuple(int(v) for v in stats)


def hypergeom_sf(x, M, n, N) -> float:
    """hyper_geom(x, M, n, N) of scaffoldToChromosomes.py:352-368, evaluated by libhicmi's host code."""
    return float(load().hicmi_hypergeom_sf(int(x), int(M), int(n), int(N)))


def hypergeom_decide(x, M, n, N, psig) -> int:
    """1 / 0 / -1: hyper_geom(x, M, n, N) < psig, >= psig, NaN - the early-exit comparison the scan kernels make."""
    return int(load().hicmi_hypergeom_decide(int(x), int(M), int(n), int(N), float(psig)))


class Context:
    """One GPU context (hicmi_ctx): owns the device-resident contact matrix and all stage buffers."""

    def __init__(self, device: int = 0):
        self._lib = load()
        h = _vp()
        _check(self._lib.hicmi_create(int(device), ctypes.byref(h)))
        self._h = h
        self.device = int(device)
        self.n = 0
        self._keepalive = None
        self._workers = []
        self._n_window_cand = 0
        self._lv_m = 0                          # nodes of the Louvain graph on the device
        self.shard = (0, 1)
        self._pairs_scaffolds = 0               # scaffolds of the resident pair store (0: this binding opened none)

    def close(self):
        for w in getattr(self, "_workers", []):
            w.close()
        self._workers = []
        if getattr(self, "_h", None):
            self._lib.hicmi_destroy(self._h)
            self._h = None

    def workers(self, count: int):
        """``count`` extra contexts on the same GPU that share this context's contact matrix (no
        copy): independent work units - Part 2's chromosomes - run on them from host threads."""
        pool = getattr(self, "_workers", None)
        if pool is None:
            pool = self._workers = []
        ptr, n, ld = _vp(), c_i64(), c_i64()
        _check(self._lib.hicmi_contacts_device(self._h, ctypes.byref(ptr), ctypes.byref(n), ctypes.byref(ld)))
        while len(pool) < count:
            pool.append(Context(self.device))
        for w in pool[:count]:
            if getattr(w, "_shared_from", None) != (ptr.value, n.value, ld.value):
                w.set_contacts_device(ptr.value, n.value, ld.value, keepalive=self)
                w._shared_from = (ptr.value, n.value, ld.value)
        return pool[:count]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _matrix_replaced(self):
        """The context is about to hold another matrix: the library forgets everything derived from the old one
        (include/hicmi.h, "What a new matrix invalidates"), and so does this binding - its note of the arrangement on the
        device, by which p2_set_arrangement skips an upload, goes with it."""
        self._arr_sig = None

    # ---- contacts
    def set_contacts(self, mat: np.ndarray):
        """Upload a square contact matrix: fp64, or fp32 (widened on the device, half the transfer)."""
        if isinstance(mat, np.ndarray) and mat.dtype == np.float32:
            mat = np.ascontiguousarray(mat)
            if mat.ndim != 2 or mat.shape[0] != mat.shape[1]:
                raise ValueError("contact matrix must be square")
            self._matrix_replaced()
            _check(self._lib.hicmi_set_contacts_host_f32(self._h, _ptr(mat), mat.shape[0]))
            self.n = mat.shape[0]
            return
        mat = np.ascontiguousarray(mat, dtype=np.float64)
        if mat.ndim != 2 or mat.shape[0] != mat.shape[1]:
            raise ValueError("contact matrix must be square")
        self._matrix_replaced()
        _check(self._lib.hicmi_set_contacts_host(self._h, _ptr(mat), mat.shape[0]))
        self.n = mat.shape[0]

    def set_contacts_device(self, data_ptr: int, n: int, ld: int | None = None, keepalive=None):
        self._matrix_replaced()
        _check(self._lib.hicmi_set_contacts_device(self._h, _vp(data_ptr), n, n if ld is None else ld))
        self.n = n
        self._keepalive = keepalive

    def contacts_device(self):
        """(device address, n, leading dimension) of the context's contact matrix (hicmi_contacts_device), for a
        further context on the same GPU to adopt with set_contacts_device(..., keepalive=this context)."""
        ptr, n, ld = _vp(), c_i64(), c_i64()
        _check(self._lib.hicmi_contacts_device(self._h, ctypes.byref(ptr), ctypes.byref(n), ctypes.byref(ld)))
        return ptr.value, n.value, ld.value

    def row_sums(self):
        np_sum = np.empty(self.n, np.float64)
        seq = np.empty(self.n, np.float64)
        _check(self._lib.hicmi_row_sums(self._h, _ptr(np_sum), _ptr(seq)))
        return np_sum, seq

    def set_row_shard(self, first: int, stride: int):
        """One map over several GPUs: this context handles rows first, first + stride, ... of the row-independent
        stages (hicmi_set_row_shard)."""
        _check(self._lib.hicmi_set_row_shard(self._h, int(first), int(stride)))
        self.shard = (int(first), int(stride))

    def set_row_sums(self, np_sum, seq_sum):
        a = np.ascontiguousarray(np_sum, dtype=np.float64)
        b = np.ascontiguousarray(seq_sum, dtype=np.float64)
        if len(a) != self.n or len(b) != self.n:
            raise ValueError("row sums must have n entries")
        _check(self._lib.hicmi_set_row_sums(self._h, _ptr(a), _ptr(b)))

    def compact(self, keep):
        keep = np.ascontiguousarray(keep, dtype=np.int32)
        self._matrix_replaced()
        _check(self._lib.hicmi_compact(self._h, _ptr(keep), len(keep)))
        self.n = len(keep)

    def rebin(self, group_start):
        """Sum the context's raw map to coarser bins (hicmi_rebin): coarse bin I is the fine bins
        [group_start[I], group_start[I + 1]); the m x m result replaces the context's matrix."""
        g = np.ascontiguousarray(group_start, dtype=np.int32)
        if g.ndim != 1 or len(g) < 2:
            raise ValueError("group_start must have m + 1 >= 2 entries")
        self._matrix_replaced()
        _check(self._lib.hicmi_rebin(self._h, _ptr(g), len(g) - 1))
        self.n = len(g) - 1

    def map_begin(self, sizes, resolution):
        """Open the count of a raw map from read pairs (hicmi_map_begin): scaffold s has
        ceil(sizes[s] / resolution) bins.  The context's matrix stays as it is until map_finish."""
        size = np.ascontiguousarray(sizes, dtype=np.int64)
        if size.ndim != 1:
            raise ValueError("sizes must be a vector")
        _check(self._lib.hicmi_map_begin(self._h, _ptr(size), len(size), int(resolution)))

    def map_begin_lifted(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, resolution):
        """Open the count of a map of the assembled genome (hicmi_map_begin_lifted): scaffold s lies in
        sequence lift_seq[s] (-1: dropped) at offset lift_off[s], reversed where lift_rev[s]; sequence q has
        ceil(seq_sizes[q] / resolution) bins.  map_add_pairs still takes scaffold indices and positions."""
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        _check(self._lib.hicmi_map_begin_lifted(self._h, _ptr(size), len(size), _ptr(seq), _ptr(off), _ptr(rev), _ptr(seq_size),
                                                len(seq_size), int(resolution)))

    def pair_stats(self, scaf_a, pos_a, scaf_b, pos_b, sizes, lift_seq, lift_off, lift_rev, seq_sizes, into=None):
        """The statistics of the pairs under the lift (hicmi_pair_stats), added to ``into``
        (new_pair_stats; None: fresh ones): (decay[256], seq_cis, seq_trans, unlifted[1]) as uint64."""
        sa, pa, sb, pb = _pair_arrays(scaf_a, pos_a, scaf_b, pos_b)
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        out = _pair_stats_into(into, len(seq_size))
        _check(self._lib.hicmi_pair_stats(self._h, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb), len(sa), _ptr(size), len(size), _ptr(seq),
                                          _ptr(off), _ptr(rev), _ptr(seq_size), len(seq_size), _ptr(out[0]), _ptr(out[1]),
                                          _ptr(out[2]), _ptr(out[3])))
        return out

    def map_add_pairs(self, scaf_a, pos_a, scaf_b, pos_b):
        """Count the pairs (scaffold index, 1-based position) x 2 into the open map (hicmi_map_add_pairs)."""
        sa, pa, sb, pb = _pair_arrays(scaf_a, pos_a, scaf_b, pos_b)
        _check(self._lib.hicmi_map_add_pairs(self._h, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb), len(sa)))

    def map_finish(self) -> int:
        """Close the count (hicmi_map_finish): the symmetric map replaces the context's matrix; returns the pairs added."""
        pairs = c_i64()
        self._matrix_replaced()
        _check(self._lib.hicmi_map_finish(self._h, ctypes.byref(pairs)))
        self.n = self.contacts_device()[1]
        self._keepalive = None
        return pairs.value

    def span_begin(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, step, max_span: int = 0):
        """Open a spanning-depth build (hicmi_span_begin) over the assembly of the lift tables, cut into cells
        of ``step`` bp; pairs further apart than ``max_span`` (0: no limit) will not count.  Returns cell_first int64[S]: the
        first cell of every scaffold, -1 for a dropped or empty one.  The matrix and an open map build are untouched."""
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        cell_first, n_cells = np.zeros(len(size), np.int64), c_i64()
        _check(self._lib.hicmi_span_begin(self._h, _ptr(size), len(size), _ptr(seq), _ptr(off), _ptr(rev), _ptr(seq_size),
                                          len(seq_size), int(step), int(max_span), _ptr(cell_first), ctypes.byref(n_cells)))
        self._span_cells = n_cells.value
        return cell_first

    def span_add_pairs(self, scaf_a, pos_a, scaf_b, pos_b):
        """Mark the pairs (scaffold index, 1-based position) x 2 in the open span build (hicmi_span_add_pairs)."""
        sa, pa, sb, pb = _pair_arrays(scaf_a, pos_a, scaf_b, pos_b)
        _check(self._lib.hicmi_span_add_pairs(self._h, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb), len(sa)))

    def span_finish(self, flank, recs, want_depth: bool = True):
        """Close the span build (hicmi_span_finish): (picks int64[n_rec, 4] = (slot, D, Lsum, Rsum) of the records
        (lo, hi, q0, q1), counters uint64[5] = (marked, one_cell, beyond_max_span, trans, unlifted), depth uint64[n_cells] or
        None).  A refused flank or record leaves the build open."""
        rec, picks = _span_records(recs)
        counters = np.zeros(5, np.uint64)
        depth = np.zeros(max(getattr(self, "_span_cells", 0), 1), np.uint64) if want_depth else None
        _check(self._lib.hicmi_span_finish(self._h, int(flank), _ptr(rec), len(rec), _ptr(picks), _ptr(counters), _ptr(depth)))
        return picks, counters, None if depth is None else depth[:self._span_cells]

    def ends_begin(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window, reach):
        """Open an end-support build (hicmi_ends_begin) over the assembly of the lift tables: end zones of
        ``window`` bases, scaffolds up to ``reach`` ranks apart.  Returns rank int32[S]: the rank of every placed scaffold, -1
        for a dropped or empty one.  The matrix, an open map build and an open span build are untouched."""
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        rank, n_placed = np.zeros(len(size), np.int32), c_i64()
        _check(self._lib.hicmi_ends_begin(self._h, _ptr(size), len(size), _ptr(seq), _ptr(off), _ptr(rev), _ptr(seq_size),
                                          len(seq_size), int(window), int(reach), _ptr(rank), ctypes.byref(n_placed)))
        self._ends_shape = (n_placed.value, int(reach), 4)
        return rank

    def ends_add_pairs(self, scaf_a, pos_a, scaf_b, pos_b):
        """Count the pairs (scaffold index, 1-based position) x 2 in the open ends build (hicmi_ends_add_pairs)."""
        sa, pa, sb, pb = _pair_arrays(scaf_a, pos_a, scaf_b, pos_b)
        _check(self._lib.hicmi_ends_add_pairs(self._h, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb), len(sa)))

    def ends_finish(self):
        """Close the ends build (hicmi_ends_finish): (table uint64[P, reach, 4], counters uint64[6] = (linked, middle, same,
        too_far, trans, unlifted))."""
        table = np.zeros(getattr(self, "_ends_shape", None) or (1, 1, 4), np.uint64)
        counters = np.zeros(6, np.uint64)
        _check(self._lib.hicmi_ends_finish(self._h, _ptr(table), _ptr(counters)))
        self._ends_shape = None
        return table, counters

    def anchor_begin(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window):
        """Open an anchor build (hicmi_anchor_begin) over the assembly of the lift tables.  ``target`` None:
        sequence mode, every dropped scaffold of size > 0 against every sequence; else rank mode, the scaffolds with a target
        >= 0 against the end zones of ``window`` bases of the placed scaffolds of that sequence.  Returns first int64[S]: the
        offset of every candidate's block of counters, -1 for a scaffold that is none.  The matrix, an open map build, an
        open span build and an open ends build are untouched."""
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        tgt = _anchor_target(target, len(size))
        first, n_table = np.zeros(len(size), np.int64), c_i64()
        _check(self._lib.hicmi_anchor_begin(self._h, _ptr(size), len(size), _ptr(seq), _ptr(off), _ptr(rev), _ptr(seq_size),
                                            len(seq_size), _ptr(tgt), int(window), _ptr(first), ctypes.byref(n_table)))
        self._anchor_cells = n_table.value
        return first

    def anchor_add_pairs(self, scaf_a, pos_a, scaf_b, pos_b):
        """Count the pairs (scaffold index, 1-based position) x 2 in the open anchor build (hicmi_anchor_add_pairs)."""
        sa, pa, sb, pb = _pair_arrays(scaf_a, pos_a, scaf_b, pos_b)
        _check(self._lib.hicmi_anchor_add_pairs(self._h, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb), len(sa)))

    def anchor_finish(self):
        """Close the anchor build (hicmi_anchor_finish): (table uint64[n_table], counters uint64[6] = (anchored, middle,
        elsewhere, skipped, unplaced, placed))."""
        table = np.zeros(getattr(self, "_anchor_cells", None) or 1, np.uint64)
        counters = np.zeros(6, np.uint64)
        _check(self._lib.hicmi_anchor_finish(self._h, _ptr(table), _ptr(counters)))
        self._anchor_cells = None
        return table, counters

    def pairs_begin(self, sizes):
        """Open an empty resident pair store (hicmi_pairs_begin) for the scaffolds of ``sizes``.  Refused when
        the context has one already.  The matrix and every open build are untouched."""
        size = np.ascontiguousarray(sizes, dtype=np.int64)
        _check(self._lib.hicmi_pairs_begin(self._h, _ptr(size), len(size)))
        self._pairs_scaffolds = len(size)

    def pairs_add(self, scaf_a, pos_a, scaf_b, pos_b):
        """Append the pairs (scaffold index, 1-based position) x 2 that lie on two scaffolds to the store and count the
        others per scaffold (hicmi_pairs_add)."""
        sa, pa, sb, pb = _pair_arrays(scaf_a, pos_a, scaf_b, pos_b)
        _check(self._lib.hicmi_pairs_add(self._h, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb), len(sa)))

    def pairs_info(self):
        """(pairs kept, intra pairs, intra uint64[S]) of the store (hicmi_pairs_info)."""
        n_kept, n_intra = c_i64(), ctypes.c_uint64()
        # intra[] is asked for only from a store this binding opened, whose scaffold count it therefore knows
        intra = np.zeros(self._pairs_scaffolds, np.uint64) if self._pairs_scaffolds else None
        _check(self._lib.hicmi_pairs_info(self._h, ctypes.byref(n_kept), ctypes.byref(n_intra), _ptr(intra)))
        return n_kept.value, n_intra.value, intra

    def pairs_fetch(self):
        """The store, downloaded (hicmi_pairs_fetch): (scaf_a int32, pos_a int64, scaf_b int32, pos_b int64)."""
        n = self.pairs_info()[0]
        sa, sb = np.zeros(n, np.int32), np.zeros(n, np.int32)
        pa, pb = np.zeros(n, np.int64), np.zeros(n, np.int64)
        _check(self._lib.hicmi_pairs_fetch(self._h, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb)))
        return sa, pa, sb, pb

    def pairs_drop(self):
        """Release the store (hicmi_pairs_drop)."""
        _check(self._lib.hicmi_pairs_drop(self._h))
        self._pairs_scaffolds = 0

    def pairs_file(self, path, names, sizes, threads: int = 0):
        """``pairs_file`` of this module on this context."""
        return pairs_file(path, names, sizes, self, threads=threads)

    def ends_resident(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window, reach):
        """End support of an assembly from the resident pair store (hicmi_ends_resident): what ``ends_file``
        returns without the parser's sums, (rank int32[S], table uint64[P, reach, 4], counters uint64[6]).  The store is
        only read; refused while an ends build is open."""
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        counters = np.zeros(6, np.uint64)
        rank, n_placed = np.zeros(len(size), np.int32), c_i64()
        table = _ends_table(ends_placed_count(size, seq), reach)
        _check(self._lib.hicmi_ends_resident(self._h, _ptr(size), len(size), _ptr(seq), _ptr(off), _ptr(rev), _ptr(seq_size),
                                             len(seq_size), int(window), int(reach), _ptr(table), _ptr(counters), _ptr(rank),
                                             ctypes.byref(n_placed)))
        if n_placed.value != table.shape[0]:
            raise RuntimeError("hicmi_ends_resident placed %d scaffolds, this binding %d" % (n_placed.value, table.shape[0]))
        return rank, table, counters

    def anchor_resident(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window):
        """Anchoring from the resident pair store (hicmi_anchor_resident): what ``anchor_file`` returns without
        the parser's sums, (first int64[S], table uint64[n_table], counters uint64[6]).  The store is only read; refused
        while an anchor build is open."""
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        tgt = _anchor_target(target, len(size))
        counters = np.zeros(6, np.uint64)
        first, n_table = np.zeros(len(size), np.int64), c_i64()
        table = _anchor_table(anchor_blocks(size, seq, len(seq_size), tgt)[1])
        _check(self._lib.hicmi_anchor_resident(self._h, _ptr(size), len(size), _ptr(seq), _ptr(off), _ptr(rev), _ptr(seq_size),
                                               len(seq_size), _ptr(tgt), int(window), _ptr(table), _ptr(counters), _ptr(first),
                                               ctypes.byref(n_table)))
        if n_table.value != len(table):
            raise RuntimeError("hicmi_anchor_resident has a table of %d counters, this binding %d" % (n_table.value, len(table)))
        return first, table, counters

    def seats_resident(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window):
        """Seat support from the resident pair store (hicmi_seats_resident): for every placed scaffold what
        ``anchor_resident`` would count in both of its modes if that scaffold alone were dropped.  Returns (first int64[S],
        table uint64[n_table], counters uint64[5] = (seated, middle, trans, same, unlifted)).  The store is only read."""
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        counters = np.zeros(5, np.uint64)
        first, n_table = np.zeros(len(size), np.int64), c_i64()
        n_counters = seats_blocks(size, seq, len(seq_size))[1]
        table = np.zeros(n_counters if 1 <= n_counters <= SEATS_MAX_TABLE else 1, np.uint64)
        _check(self._lib.hicmi_seats_resident(self._h, _ptr(size), len(size), _ptr(seq), _ptr(off), _ptr(rev), _ptr(seq_size),
                                              len(seq_size), int(window), _ptr(table), _ptr(counters), _ptr(first),
                                              ctypes.byref(n_table)))
        if n_table.value != len(table):
            raise RuntimeError("hicmi_seats_resident has a table of %d counters, this binding %d" % (n_table.value, len(table)))
        return first, table, counters

    def links_resident(self, sizes, window):
        """The end-link graph of all scaffolds from the resident pair store (hicmi_links_resident and hicmi_links_fetch,
        DESIGN.md 9t): one row per scaffold pair with at least one kept pair, sorted by (lo, hi).  Returns (lo int32[E],
        hi int32[E], counts uint64[E, 5] in the order LL, LR, RL, RR, OTHER - first letter: the end zone on ``lo`` -
        counters uint64[2] = (linked, middle)).  No order file takes part; the store is only read."""
        size = np.ascontiguousarray(sizes, dtype=np.int64)
        counters, n_rows = np.zeros(2, np.uint64), c_i64()
        _check(self._lib.hicmi_links_resident(self._h, _ptr(size), len(size), int(window), ctypes.byref(n_rows), _ptr(counters)))
        lo, hi = np.zeros(n_rows.value, np.int32), np.zeros(n_rows.value, np.int32)
        counts = np.zeros((n_rows.value, 5), np.uint64)
        _check(self._lib.hicmi_links_fetch(self._h, _ptr(lo), _ptr(hi), _ptr(counts)))
        return lo, hi, counts, counters

    def links_lifted(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window):
        """The end-link graph between the ends of sequences that consist of several scaffolds (hicmi_links_lifted and
        hicmi_links_fetch): ``links_resident`` with both ends of every pair lifted onto the sequences first.
        Returns (lo int32[E], hi int32[E], counts uint64[E, 5], counters uint64[4] = (linked, middle, inside, unlifted));
        ``lo`` and ``hi`` are sequence indices.  The store is only read."""
        size, seq, off, rev, seq_size = _lift_tables(sizes, lift_seq, lift_off, lift_rev, seq_sizes)
        counters, n_rows = np.zeros(4, np.uint64), c_i64()
        _check(self._lib.hicmi_links_lifted(self._h, _ptr(size), len(size), _ptr(seq), _ptr(off), _ptr(rev), _ptr(seq_size),
                                            len(seq_size), int(window), ctypes.byref(n_rows), _ptr(counters)))
        lo, hi = np.zeros(n_rows.value, np.int32), np.zeros(n_rows.value, np.int32)
        counts = np.zeros((n_rows.value, 5), np.uint64)
        _check(self._lib.hicmi_links_fetch(self._h, _ptr(lo), _ptr(hi), _ptr(counts)))
        return lo, hi, counts, counters

    def links_info(self):
        """(records, slots, sort_ms) of the last ``links_resident`` or ``links_lifted`` call (hicmi_links_info): the used slots of its table, the
        slots the table had, and the milliseconds the host took to sort the records."""
        n_rec, n_slots, ms = c_i64(), c_i64(), ctypes.c_double()
        _check(self._lib.hicmi_links_info(self._h, ctypes.byref(n_rec), ctypes.byref(n_slots), ctypes.byref(ms)))
        return n_rec.value, n_slots.value, ms.value

    def split_pairs(self, scaf_a, pos_a, scaf_b, pos_b, sizes, piece_first, piece_start, into=None):
        """The pairs (scaffold index, 1-based position) x 2 moved to the pieces the scaffolds are cut into
        (hicmi_split_pairs): (piece a, position a, piece b, position b, counters), the counters uint64[4,
        n_piece] = (within, sibling, other, mark) added to ``into`` (new_split_counters; None: fresh ones).  The matrix, an
        open map build and an open span build are untouched."""
        sa, pa, sb, pb = _pair_arrays(scaf_a, pos_a, scaf_b, pos_b)
        size, first, start = _split_tables(sizes, piece_first, piece_start)
        out = _split_counters_into(into, len(start))
        ka, kb, xa, xb = np.empty_like(sa), np.empty_like(sb), np.empty_like(pa), np.empty_like(pb)
        _check(self._lib.hicmi_split_pairs(self._h, _ptr(sa), _ptr(pa), _ptr(sb), _ptr(pb), len(sa), _ptr(size), len(size),
                                           _ptr(first), _ptr(start), len(start), _ptr(ka), _ptr(xa), _ptr(kb), _ptr(xb), _ptr(out)))
        return ka, xa, kb, xb, out

    def group_sums(self, grp, scaf, n_groups, n_scaffolds, want_bins=True):
        """Group support sums (hicmi_group_sums): (bin sums n x n_groups or None, scaffold sums
        n_scaffolds x n_groups) for the group label (-1: none) and the dense scaffold id of every bin."""
        g = np.ascontiguousarray(grp, dtype=np.int32)
        s = np.ascontiguousarray(scaf, dtype=np.int32)
        if g.shape != (self.n,) or s.shape != (self.n,):
            raise ValueError("grp and scaf must have n entries")
        bins = np.empty((self.n, int(n_groups)), np.float64) if want_bins else None
        scaffolds = np.empty((int(n_scaffolds), int(n_groups)), np.float64)
        _check(self._lib.hicmi_group_sums(self._h, _ptr(g), _ptr(s), int(n_groups), int(n_scaffolds), _ptr(bins),
                                          _ptr(scaffolds)))
        return bins, scaffolds

    def junction_sums(self, bins, rec):
        """Junction sums (hicmi_junction_sums): for every row (startA, stepA, lenA, startB, stepB, lenB)
        of ``rec``, the sum of M[A_a][B_b] / (a + b + 1) over its two sides, views of ``bins`` (matrix indices)."""
        b = np.ascontiguousarray(bins, dtype=np.int32)
        r = np.ascontiguousarray(rec, dtype=np.int64)
        if b.ndim != 1 or r.ndim != 2 or r.shape[1] != 6:
            raise ValueError("bins must be a vector and rec n_rec x 6")
        sums = np.empty(len(r), np.float64)
        _check(self._lib.hicmi_junction_sums(self._h, _ptr(b), len(b), _ptr(r), len(r), _ptr(sums)))
        return sums

    # ---- Part 0: ICE balancing
    def ice_mask_rows(self, mask):
        """Zero the rows and columns ``mask`` flags in the context's own matrix (hicmi_ice_mask_rows)."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.shape != (self.n,):
            raise ValueError("mask must have n entries")
        self._matrix_replaced()
        _check(self._lib.hicmi_ice_mask_rows(self._h, _ptr(m), self.n))

    def ice_balance(self, mask=None, max_iter=100, eps=0.1):
        """ICE-balance the context's own matrix in place (hicmi_ice_balance): returns (biases with nan for the masked
        bins, iterations run, last sum |bias_prev - bias|)."""
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if m is not None and m.shape != (self.n,):
            raise ValueError("mask must have n entries")
        bias = np.empty(self.n, np.float64)
        iters, delta = c_i64(0), c_dbl(0.0)
        self._matrix_replaced()
        _check(self._lib.hicmi_ice_balance(self._h, _ptr(m), int(max_iter), float(eps), _ptr(bias), ctypes.byref(iters),
                                           ctypes.byref(delta)))
        return bias, int(iters.value), delta.value

    def contacts_host(self):
        """The context's contact matrix copied to the host (hicmi_get_contact_rows): n x n fp64."""
        out = np.empty((self.n, self.n), np.float64)
        _check(self._lib.hicmi_get_contact_rows(self._h, 0, self.n, _ptr(out)))
        return out

    # ---- Part 1
    def upgma(self, want_linkage: bool = True):
        z = np.empty((max(self.n - 1, 0), 4), np.float64) if want_linkage else None
        leaves = np.empty(self.n, np.int32)
        _check(self._lib.hicmi_upgma(self._h, _ptr(z), _ptr(leaves)))
        return leaves, z

    def selftest_division(self, samples=1 << 28, seed=12345):
        bad = ctypes.c_uint64()
        _check(self._lib.hicmi_selftest_division(self._h, seed, samples, ctypes.byref(bad)))
        return bad.value

    def raw_merges(self):
        z = np.empty((max(self.n - 1, 0), 4), np.float64)
        _check(self._lib.hicmi_get_raw_merges(self._h, _ptr(z)))
        return z

    def nnchain_stats(self):
        """Counters of the nn-chain kernels since the last timing_reset (hicmi_nnchain_stats)."""
        out = np.zeros(6, np.float64)
        _check(self._lib.hicmi_nnchain_stats(self._h, _ptr(out)))
        return dict(merges=out[0], scans=out[1], scan_columns=out[2], cache_hits=out[3], retries=int(out[4]))

    def rank_matrix(self, order):
        order = np.ascontiguousarray(order, dtype=np.int32)
        if len(order) != self.n:
            raise ValueError("order must have n entries")
        _check(self._lib.hicmi_rank_matrix(self._h, _ptr(order)))

    def presort_state(self):
        """(state, tied_rows) of the last rank_matrix.  state 0: it sorted every row itself; 1: it re-addressed the
        rows sorted beside the nn-chain and sorted `tied_rows` rows (those holding equal similarities) again;
        2: more than half of the rows hold equal similarities, the pre-sort was discarded (hicmi_presort_state)."""
        st = ctypes.c_int(0)
        tied = c_i64(0)
        _check(self._lib.hicmi_presort_state(self._h, ctypes.byref(st), ctypes.byref(tied)))
        return st.value, int(tied.value)

    def rank_rows(self, row0=0, nrows=None, inverse=False):
        nrows = self.n - row0 if nrows is None else nrows
        out = np.empty((nrows, self.n), np.uint16)
        _check(self._lib.hicmi_get_rank_rows(self._h, row0, nrows, 1 if inverse else 0, _ptr(out)))
        return out

    def similarity_row(self, row):
        out = np.empty(self.n, np.float64)
        _check(self._lib.hicmi_get_similarity_row(self._h, row, _ptr(out)))
        return out

    def cut_scan(self, start, M, psig, want_x=False):
        cnt = self.n - start
        sig = np.empty(cnt, np.uint8)
        x = np.empty(cnt, np.int32) if want_x else None
        _check(self._lib.hicmi_cut_scan(self._h, start, M, psig, _ptr(x), _ptr(sig)))
        return (sig, x) if want_x else sig

    def filter_scan(self, start, c, n_rows, M, psig, want_x=False):
        sig = np.empty(n_rows, np.uint8)
        x = np.empty(n_rows, np.int32) if want_x else None
        _check(self._lib.hicmi_filter_scan(self._h, start, c, n_rows, M, psig, _ptr(x), _ptr(sig)))
        return (sig, x) if want_x else sig

    def first_pass_cuts(self, min_size, stop_ind, psig):
        """pre_process_all_matrix_breakpoints' loop on the device (hicmi_first_pass_cuts): (cuts, [(M before, M after), ...])."""
        cuts = np.empty(self.n, np.int32)
        mlog = np.empty((self.n, 2), np.int32)
        nc, nl = c_i64(0), c_i64(0)
        _check(self._lib.hicmi_first_pass_cuts(self._h, int(min_size), int(stop_ind), float(psig), _ptr(cuts), self.n,
                                               ctypes.byref(nc), _ptr(mlog), self.n, ctypes.byref(nl)))
        return [int(v) for v in cuts[:nc.value]], [(int(a), int(b)) for a, b in mlog[:nl.value]]

    def filter_cuts(self, cuts, psig):
        """filter_noisy_breakpoints' loops on the device (hicmi_filter_cuts): (sorted kept cuts, warnings)."""
        cuts = np.ascontiguousarray(cuts, dtype=np.int32)
        out = np.empty(self.n, np.int32)
        m, warned = c_i64(0), c_i64(0)
        _check(self._lib.hicmi_filter_cuts(self._h, _ptr(cuts), len(cuts), float(psig), _ptr(out), self.n,
                                           ctypes.byref(m), ctypes.byref(warned)))
        return [int(v) for v in out[:m.value]], int(warned.value)

    SCAN_MAX_SETS = 64                                     # HICMI_SCAN_MAX_SETS: larger grids go in chunks

    def first_pass_cuts_multi(self, sets, psig):
        """first_pass_cuts for many (min_size, stop_ind) sets in lock step (hicmi_first_pass_cuts_multi): one
        (cuts, [(M before, M after), ...]) per set, in order."""
        out = []
        n = self.n
        for c0 in range(0, len(sets), self.SCAN_MAX_SETS):
            part = sets[c0:c0 + self.SCAN_MAX_SETS]
            k = len(part)
            ms = np.array([int(a) for a, _b in part], np.int64)
            si = np.array([int(b) for _a, b in part], np.int64)
            cuts = np.empty((k, n), np.int32)
            mlog = np.empty((k, n, 2), np.int32)
            nc, nl = np.zeros(k, np.int64), np.zeros(k, np.int64)
            _check(self._lib.hicmi_first_pass_cuts_multi(self._h, k, _ptr(ms), _ptr(si), float(psig), _ptr(cuts), n,
                                                         _ptr(nc), _ptr(mlog), n, _ptr(nl)))
            out += [([int(v) for v in cuts[j, :nc[j]]], [(int(a), int(b)) for a, b in mlog[j, :nl[j]]]) for j in range(k)]
        return out

    def filter_cuts_multi(self, lists, psigs):
        """filter_cuts for many (candidate list, psig) sets in lock step (hicmi_filter_cuts_multi): one
        (sorted kept cuts, warnings) per set, in order.  An empty list gives ([], 0)."""
        out = []
        n = self.n
        for c0 in range(0, len(lists), self.SCAN_MAX_SETS):
            part = [np.asarray(v, dtype=np.int32) for v in lists[c0:c0 + self.SCAN_MAX_SETS]]
            k = len(part)
            off = np.zeros(k + 1, np.int64)
            off[1:] = np.cumsum([len(v) for v in part])
            cand = np.ascontiguousarray(np.concatenate(part) if off[-1] else np.zeros(1, np.int32), dtype=np.int32)
            ps = np.array([float(v) for v in psigs[c0:c0 + self.SCAN_MAX_SETS]], np.float64)
            kept = np.empty((k, n), np.int32)
            m, warned = np.zeros(k, np.int64), np.zeros(k, np.int64)
            _check(self._lib.hicmi_filter_cuts_multi(self._h, k, _ptr(off), _ptr(cand), _ptr(ps), _ptr(kept), n,
                                                     _ptr(m), _ptr(warned)))
            out += [([int(v) for v in kept[j, :m[j]]], int(warned[j])) for j in range(k)]
        return out

    # ---- Part 2
    def p2_select(self, sel):
        sel = np.ascontiguousarray(sel, dtype=np.int32)
        _check(self._lib.hicmi_p2_select(self._h, _ptr(sel), len(sel)))
        self._arr_sig = None

    def p2_total(self) -> float:
        t = c_dbl()
        _check(self._lib.hicmi_p2_total(self._h, ctypes.byref(t)))
        return t.value

    def p2_score(self, perms, total: float):
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        if perms.ndim != 2:
            raise ValueError("perms must be (n_cand, n_used)")
        out = np.empty(perms.shape[0], np.float64)
        if perms.shape[0]:
            _check(self._lib.hicmi_p2_score(self._h, _ptr(perms), perms.shape[0], perms.shape[1], float(total), _ptr(out)))
        return out

    def p2_score_exact(self, perms, total: float):
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        if perms.ndim != 2:
            raise ValueError("perms must be (n_cand, n_used)")
        out = np.empty(perms.shape[0], np.float64)
        if perms.shape[0]:
            _check(self._lib.hicmi_p2_score_exact(self._h, _ptr(perms), perms.shape[0], perms.shape[1], float(total),
                                                  _ptr(out)))
        return out

    # ---- Part 2 search with device-side enumeration
    def p2_layout(self, scaf_start, scaf_len):
        a = np.ascontiguousarray(scaf_start, dtype=np.int32)
        b = np.ascontiguousarray(scaf_len, dtype=np.int32)
        _check(self._lib.hicmi_p2_layout(self._h, _ptr(a), _ptr(b), len(a)))
        self._arr_sig = None

    def p2_set_arrangement(self, ids, rev):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        b = np.ascontiguousarray(rev, dtype=np.uint8)
        sig = a.tobytes() + b.tobytes()
        if sig == getattr(self, "_arr_sig", None):
            return                                   # the device already holds this arrangement
        _check(self._lib.hicmi_p2_set_arrangement(self._h, _ptr(a), _ptr(b), len(a)))
        self._arr_len = len(a)
        self._arr_sig = sig

    def p2_arrangement_total(self) -> float:
        t = c_dbl()
        _check(self._lib.hicmi_p2_arrangement_total(self._h, ctypes.byref(t)))
        return t.value

    def p2_arrangement_score(self, total: float) -> float:
        t = c_dbl()
        _check(self._lib.hicmi_p2_arrangement_score(self._h, float(total), ctypes.byref(t)))
        return t.value

    def p2_score_insertions(self, new_id: int, total: float):
        out = np.empty(2 * (self._arr_len + 1), np.float64)
        _check(self._lib.hicmi_p2_score_insertions(self._h, int(new_id), float(total), _ptr(out)))
        return out

    def p2_window_tables(self, orders, orients):
        a = np.ascontiguousarray(orders, dtype=np.int8)
        b = np.ascontiguousarray(orients, dtype=np.uint8)
        _check(self._lib.hicmi_p2_window_tables(self._h, a.shape[1], _ptr(a), a.shape[0], _ptr(b), b.shape[0]))
        self._n_window_cand = a.shape[0] * b.shape[0]

    def p2_score_window(self, first: int, k: int):
        if not self._n_window_cand:
            raise HicmiError("p2_window_tables has not been called")
        out = np.empty(self._n_window_cand, np.float64)
        _check(self._lib.hicmi_p2_score_window(self._h, int(first), int(k), _ptr(out)))
        return out

    def p2_decide_window(self, first, k, total, floor, cur_fast):
        """One whole window step; returns (pick or -1, literal best, fast score of the resulting arrangement)."""
        pick, best, pf = c_i64(), c_dbl(), c_dbl()
        _check(self._lib.hicmi_p2_decide_window(self._h, int(first), int(k), float(total), float(floor),
                                                float("nan") if cur_fast is None else float(cur_fast),
                                                ctypes.byref(pick), ctypes.byref(best), ctypes.byref(pf)))
        return pick.value, best.value, pf.value

    def p2_window_shortlist(self, first, count, k, total, floor, cur_fast=None, cap=4096):
        """Device short lists of ``count`` consecutive windows (hicmi_p2_window_shortlist): per window
        (candidate indices, fast scores), or None when its list overflowed ``cap``."""
        n_near = np.zeros(int(count), np.int64)
        idx = np.zeros((int(count), int(cap)), np.int64)
        fast = np.zeros((int(count), int(cap)), np.float64)
        _check(self._lib.hicmi_p2_window_shortlist(self._h, int(first), int(count), int(k), float(total), float(floor),
                                                   float("nan") if cur_fast is None else float(cur_fast), int(cap),
                                                   _ptr(n_near), _ptr(idx), _ptr(fast)))
        return [None if m > cap else (idx[w, :m].copy(), fast[w, :m].copy()) for w, m in enumerate(n_near.tolist())]

    def p2_decide_insertion(self, ids, rev, new_id, new_rev_now):
        """One whole checkAllScores step; returns (gap or -1, reversed flag, literal best)."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        b = np.ascontiguousarray(rev, dtype=np.uint8)
        gap, r, best = c_i64(), ctypes.c_int32(), c_dbl()
        _check(self._lib.hicmi_p2_decide_insertion(self._h, _ptr(a), _ptr(b), len(a), int(new_id), int(new_rev_now),
                                                   ctypes.byref(gap), ctypes.byref(r), ctypes.byref(best)))
        self._arr_sig = a.tobytes() + b.tobytes()
        self._arr_len = len(a)
        return gap.value, r.value, best.value

    def p2_insert_all(self, ids, rev, new_ids):
        """orderRemainderScaffolds in one call; returns (ids, rev, bestCost of the last insertion)."""
        s0, k = len(ids), len(new_ids)
        a = np.zeros(s0 + k, np.int32); a[:s0] = ids
        b = np.zeros(s0 + k, np.uint8); b[:s0] = rev
        nw = np.ascontiguousarray(new_ids, dtype=np.int32)
        best = c_dbl()
        _check(self._lib.hicmi_p2_insert_all(self._h, _ptr(a), _ptr(b), s0, _ptr(nw), k, ctypes.byref(best)))
        self._arr_sig = None
        return a, b, best.value

    @staticmethod
    def p2_insert_all_multi(jobs):
        """orderRemainderScaffolds for several chromosomes in lock step (hicmi_p2_insert_all_multi).
        jobs: [(context, ids, rev, new_ids)], one distinct context per chromosome; returns
        [(ids, rev, bestCost of the last insertion)] in the same order."""
        n = len(jobs)
        if n == 0:
            return []
        lib = jobs[0][0]._lib
        keep, a_l, b_l, nw_l = [], [], [], []
        for ctx, ids, rev, new_ids in jobs:
            s0, k = len(ids), len(new_ids)
            a = np.zeros(s0 + k, np.int32); a[:s0] = ids
            b = np.zeros(s0 + k, np.uint8); b[:s0] = rev
            a_l.append(a); b_l.append(b); nw_l.append(np.ascontiguousarray(new_ids, dtype=np.int32))
        handles = (ctypes.c_void_p * n)(*[j[0]._h for j in jobs])
        pa = (ctypes.c_void_p * n)(*[x.ctypes.data for x in a_l])
        pb = (ctypes.c_void_p * n)(*[x.ctypes.data for x in b_l])
        pn = (ctypes.c_void_p * n)(*[x.ctypes.data for x in nw_l])
        s0s = (c_i64 * n)(*[len(j[1]) for j in jobs])
        ks = (c_i64 * n)(*[len(j[3]) for j in jobs])
        best = (c_dbl * n)()
        _check(lib.hicmi_p2_insert_all_multi(n, handles, pa, pb, s0s, pn, ks, best))
        for ctx, _i, _r, _n in jobs:
            ctx._arr_sig = None
        return [(a_l[j], b_l[j], best[j]) for j in range(n)]

    @staticmethod
    def p2_start_all(jobs, tables):
        """The start phase of several chromosomes in one call (hicmi_p2_start_all).  jobs: [(context, sel, scaf_start,
        scaf_len, first_ids)], one distinct context per chromosome; tables: {k: (orders, orients as 0 / 1)} for every
        k = len(first_ids) that occurs.  Returns [(total, pick or -1, literal cost, status)]; status 0 decided, 1 total is
        0 (nothing scored), 2 no candidate above 0."""
        n = len(jobs)
        if n == 0:
            return []
        lib = jobs[0][0]._lib
        i32 = lambda col: np.ascontiguousarray(np.concatenate([np.asarray(j[col], dtype=np.int32) for j in jobs]), dtype=np.int32)
        sel, st, ln, ids = i32(1), i32(2), i32(3), i32(4)
        n_sel = (c_i64 * n)(*[len(j[1]) for j in jobs])
        n_scaf = (c_i64 * n)(*[len(j[2]) for j in jobs])
        ks = (c_i64 * n)(*[len(j[4]) for j in jobs])
        keep = {k: (np.ascontiguousarray(o, dtype=np.int8), np.ascontiguousarray(r, dtype=np.uint8)) for k, (o, r) in tables.items()}
        po = (ctypes.c_void_p * 9)(*[keep[k][0].ctypes.data if k in keep else None for k in range(9)])
        pr = (ctypes.c_void_p * 9)(*[keep[k][1].ctypes.data if k in keep else None for k in range(9)])
        no = (c_i64 * 9)(*[keep[k][0].shape[0] if k in keep else 0 for k in range(9)])
        nr = (c_i64 * 9)(*[keep[k][1].shape[0] if k in keep else 0 for k in range(9)])
        handles = (ctypes.c_void_p * n)(*[j[0]._h for j in jobs])
        total, pick, cost, status = (c_dbl * n)(), (c_i64 * n)(), (c_dbl * n)(), (ctypes.c_int32 * n)()
        _check(lib.hicmi_p2_start_all(n, handles, _ptr(sel), n_sel, _ptr(st), _ptr(ln), n_scaf, _ptr(ids), ks, po, no, pr, nr,
                                      total, pick, cost, status))
        for j, job in enumerate(jobs):
            ctx, k = job[0], len(job[4])
            ctx._arr_sig, ctx._arr_len = None, k
            if status[j] != 1:
                ctx._n_window_cand = keep[k][0].shape[0] * keep[k][1].shape[0]
        return [(total[j], int(pick[j]), cost[j], int(status[j])) for j in range(n)]

    def p2_scan_arranged(self, ids, rev, k, orders, orients, best):
        """scanOrdering from the arrangement the insertion phase returned (hicmi_p2_scan_arranged): returns (ids, rev,
        best, rounds, total)."""
        a = np.ascontiguousarray(ids, dtype=np.int32).copy()
        b = np.ascontiguousarray(rev, dtype=np.uint8).copy()
        o = np.ascontiguousarray(orders, dtype=np.int8)
        r = np.ascontiguousarray(orients, dtype=np.uint8)
        bst, total, rounds = c_dbl(float(best)), c_dbl(), c_i64()
        _check(self._lib.hicmi_p2_scan_arranged(self._h, _ptr(a), _ptr(b), len(a), int(k), _ptr(o), o.shape[0], _ptr(r), r.shape[0],
                                                ctypes.byref(total), ctypes.byref(bst), ctypes.byref(rounds)))
        self._arr_sig = None
        self._n_window_cand = o.shape[0] * r.shape[0]
        return a, b, bst.value, int(rounds.value), total.value

    def _table_call(self, fn, ids, rev, table, args):
        """One chromosome's table call: hicmi_p2_support / hicmi_p2_breaks(handle, ids, rev, S, *args, table, best)."""
        a = np.ascontiguousarray(ids, dtype=np.int32)
        b = np.ascontiguousarray(rev, dtype=np.uint8)
        best = np.empty((len(a), 2), np.int32)
        _check(fn(self._h, _ptr(a), _ptr(b), len(a), *args, _ptr(table), _ptr(best)))
        self._arr_sig, self._arr_len = a.tobytes() + b.tobytes(), len(a)
        return table, best

    @staticmethod
    def _table_multi(fn_name, jobs, totals, shape_of, args=()):
        """The marshalling of hicmi_p2_support_multi / hicmi_p2_breaks_multi: jobs [(context, ids, rev, ...)], one table of
        ``shape_of(job, S)`` per job, ``args`` between the totals and the outputs; returns [(table, best)]."""
        n = len(jobs)
        if n == 0:
            return []
        a_l = [np.ascontiguousarray(j[1], dtype=np.int32) for j in jobs]
        b_l = [np.ascontiguousarray(j[2], dtype=np.uint8) for j in jobs]
        t_l = [np.empty(shape_of(j, len(a)), np.float64) for j, a in zip(jobs, a_l)]
        o_l = [np.empty((len(a), 2), np.int32) for a in a_l]
        handles = (ctypes.c_void_p * n)(*[j[0]._h for j in jobs])
        pa, pb, pt, po = ((ctypes.c_void_p * n)(*[x.ctypes.data for x in arrs]) for arrs in (a_l, b_l, t_l, o_l))
        sizes = (c_i64 * n)(*[len(a) for a in a_l])
        _check(getattr(jobs[0][0]._lib, fn_name)(n, handles, pa, pb, sizes, (c_dbl * n)(*map(float, totals)), *args, pt, po))
        for j, a, b in zip(jobs, a_l, b_l):
            j[0]._arr_sig, j[0]._arr_len = a.tobytes() + b.tobytes(), len(a)
        return list(zip(t_l, o_l))

    def p2_support(self, ids, rev, total: float):
        """Placement support of one chromosome (hicmi_p2_support): (S x S x 2 table of closed-form scores,
        S x 2 int32 of [first maximum 2 g + r among the candidates that differ from the arrangement or -1,
        how many of them lie within 1e-9 of it])."""
        return self._table_call(self._lib.hicmi_p2_support, ids, rev, np.empty((len(ids), len(ids), 2), np.float64), (float(total),))

    @staticmethod
    def p2_support_multi(jobs):
        """p2_support for several chromosomes in one pair of launches (hicmi_p2_support_multi).
        jobs: [(context, ids, rev, total)], one distinct context per chromosome; returns [(table, best)]."""
        return Context._table_multi("hicmi_p2_support_multi", jobs, [j[3] for j in jobs], lambda j, S: (S, S, 2))

    def p2_breaks(self, ids, rev, lengths, total: float, min_piece: int = 1):
        """Break support of one chromosome (hicmi_p2_breaks): see p2_breaks_multi."""
        table = np.empty((sum(max(int(ln) - 1, 0) for ln in lengths), 8), np.float64)
        return self._table_call(self._lib.hicmi_p2_breaks, ids, rev, table, (float(total), int(min_piece)))

    @staticmethod
    def p2_breaks_multi(jobs, min_piece: int = 1):
        """Break support of several chromosomes in one pair of launches (hicmi_p2_breaks_multi).
        jobs: [(context, ids, rev, lengths, total)], one distinct context per chromosome, ``lengths`` the bins of each
        scaffold of the arrangement; returns [(table, best)]: the scaffolds' (L - 1) x 8 blocks of closed-form scores
        concatenated in arrangement order as one (sum of L - 1) x 8 array, and S x 2 int32 of [8 (p - 1) + k of the first
        maximum among the competing candidates or -1, how many of them lie within 1e-9 of it]."""
        return Context._table_multi("hicmi_p2_breaks_multi", jobs, [j[4] for j in jobs],
                                    lambda j, S: (sum(max(int(ln) - 1, 0) for ln in j[3]), 8), (int(min_piece),))

    def p2_inversions(self, ids, rev, total: float, max_span: int = 0):
        """Inversion support of one chromosome (hicmi_p2_inversions): see p2_inversions_multi."""
        return self._table_call(self._lib.hicmi_p2_inversions, ids, rev, np.empty((len(ids), len(ids)), np.float64),
                                (float(total), int(max_span)))

    @staticmethod
    def p2_inversions_multi(jobs, max_span: int = 0):
        """Inversion support of several chromosomes in one pair of launches (hicmi_p2_inversions_multi).
        jobs: [(context, ids, rev, total)], one distinct context per chromosome; returns [(table, best)]: the S x S
        closed-form scores of "scaffolds i ... j reversed and flipped" (row i, column j; 0.0 for j < i and beyond
        ``max_span`` scaffolds) and S x 2 int32 of [j of the first maximum among the competing candidates with left end i
        or -1, how many of them lie within 1e-9 of it]."""
        return Context._table_multi("hicmi_p2_inversions_multi", jobs, [j[3] for j in jobs], lambda j, S: (S, S),
                                    (int(max_span),))

    def p2_scan_pass(self, ids, rev, k, total, best, cur_fast):
        """One round of scanOrdering; returns (ids, rev, best, cur_fast, improved)."""
        a = np.ascontiguousarray(ids, dtype=np.int32).copy()
        b = np.ascontiguousarray(rev, dtype=np.uint8).copy()
        bst = c_dbl(float(best))
        cf = c_dbl(float("nan") if cur_fast is None else float(cur_fast))
        imp = ctypes.c_int32()
        _check(self._lib.hicmi_p2_scan_pass(self._h, _ptr(a), _ptr(b), len(a), int(k), float(total), ctypes.byref(bst),
                                            ctypes.byref(cf), ctypes.byref(imp)))
        self._arr_sig = None
        return a, b, bst.value, cf.value, bool(imp.value)

    def p2_scan_all(self, ids, rev, k, total, best, cur_fast):
        """scanOrdering's rounds until one brings no improvement; returns (ids, rev, best, cur_fast, rounds)."""
        a = np.ascontiguousarray(ids, dtype=np.int32).copy()
        b = np.ascontiguousarray(rev, dtype=np.uint8).copy()
        bst = c_dbl(float(best))
        cf = c_dbl(float("nan") if cur_fast is None else float(cur_fast))
        rounds = c_i64()
        _check(self._lib.hicmi_p2_scan_all(self._h, _ptr(a), _ptr(b), len(a), int(k), float(total), ctypes.byref(bst),
                                           ctypes.byref(cf), ctypes.byref(rounds)))
        self._arr_sig = None
        return a, b, bst.value, cf.value, int(rounds.value)

    # ---- plot support
    def plot_percentiles(self, kind, order, q):
        """numpy.percentile (linear) of the cells of the (transformed) matrix restricted to ``order``."""
        qa = np.ascontiguousarray(q, dtype=np.float64)
        out = np.empty(len(qa), np.float64)
        if order is None:
            n_sel, optr, keep = self.n, None, None
        else:
            keep = np.ascontiguousarray(order, dtype=np.int32)
            n_sel, optr = len(keep), _ptr(keep)
        _check(self._lib.hicmi_plot_percentiles(self._h, int(kind), optr, n_sel, _ptr(qa), len(qa), _ptr(out)))
        return out

    def plot_downsample(self, kind, order, px):
        """px x px block means of the (transformed) matrix restricted / permuted by ``order``."""
        if order is None:
            n_sel, optr, keep = self.n, None, None
        else:
            keep = np.ascontiguousarray(order, dtype=np.int32)
            n_sel, optr = len(keep), _ptr(keep)
        out = np.empty((int(px), int(px)), np.float64)
        _check(self._lib.hicmi_plot_downsample(self._h, int(kind), optr, n_sel, int(px), _ptr(out)))
        return out

    # ---- HMM boundary finder (hmm = True, S2C:730-942)
    def hmm_load_obs(self, order, c, p):
        """X = log10(similarity + 1) of rows [c, n) and columns [c, p) in ``order``, kept on the device.
        Returns (T, D)."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        _check(self._lib.hicmi_hmm_load_obs(self._h, _ptr(order), len(order), int(c), int(p)))
        self._hmm_shape = [len(order) - int(c), int(p) - int(c), int(p) - int(c)]      # T, built width, view width
        self.__dict__.setdefault("_hmm_slots", {})[0] = self._hmm_shape                # (slot 0, now selected)
        self._hmm_cur = 0
        return self._hmm_shape[0], self._hmm_shape[1]

    def hmm_set_obs(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X must be 2-D")
        _check(self._lib.hicmi_hmm_set_obs(self._h, _ptr(X), X.shape[0], X.shape[1]))
        self._hmm_shape = [X.shape[0], X.shape[1], X.shape[1]]
        self.__dict__.setdefault("_hmm_slots", {})[0] = self._hmm_shape
        self._hmm_cur = 0

    def hmm_set_width(self, D):
        """Use columns [0, D) of the X already on the device."""
        _check(self._lib.hicmi_hmm_set_width(self._h, int(D)))
        self._hmm_shape[2] = int(D)

    def hmm_get_obs(self, row0=0, nrows=None):
        T, _ld, D = self._hmm_shape
        nrows = T - row0 if nrows is None else nrows
        out = np.empty((nrows, D), np.float64)
        _check(self._lib.hicmi_hmm_get_obs(self._h, int(row0), int(nrows), _ptr(out)))
        return out

    def hmm_dist2(self, rows):
        """Squared distances of every row of X to the rows ``rows`` (1 or 2 of them): len(rows) x T."""
        r = np.ascontiguousarray(rows, dtype=np.int64)
        out = np.empty((len(r), self._hmm_shape[0]), np.float64)
        _check(self._lib.hicmi_hmm_dist2(self._h, _ptr(r), len(r), _ptr(out)))
        return out

    def hmm_col_stats(self):
        """(mean, sum of squared deviations) of every column of X."""
        D = self._hmm_shape[2]
        mean, m2 = np.empty(D, np.float64), np.empty(D, np.float64)
        _check(self._lib.hicmi_hmm_col_stats(self._h, _ptr(mean), _ptr(m2)))
        return mean, m2

    def hmm_kmeans(self, centers, max_iter=300, tol=0.0, want_labels=True):
        """Lloyd from ``centers`` (2 x D): (centers, labels or None, inertia, iterations)."""
        cin = np.ascontiguousarray(centers, dtype=np.float64)
        cout = np.empty_like(cin)
        labels = np.empty(self._hmm_shape[0], np.int32) if want_labels else None
        inertia, n_iter = c_dbl(), c_i64()
        _check(self._lib.hicmi_hmm_kmeans(self._h, _ptr(cin), int(max_iter), float(tol), _ptr(cout), _ptr(labels),
                                          ctypes.byref(inertia), ctypes.byref(n_iter)))
        return cout, labels, inertia.value, int(n_iter.value)

    def hmm_fit(self, startprob, means, covars, transmat, n_iter=1000, tol=1e-2):
        """Baum-Welch: (means, covars, transmat, logprob of every iteration)."""
        sp = np.ascontiguousarray(startprob, dtype=np.float64)
        mu = np.array(means, dtype=np.float64, order="C")
        cv = np.array(covars, dtype=np.float64, order="C")
        tm = np.array(transmat, dtype=np.float64, order="C")
        hist = np.empty(int(n_iter), np.float64)
        done = c_i64()
        _check(self._lib.hicmi_hmm_fit(self._h, _ptr(sp), _ptr(mu), _ptr(cv), _ptr(tm), int(n_iter), float(tol),
                                       _ptr(hist), ctypes.byref(done)))
        return mu, cv, tm, hist[:done.value].copy()

    def hmm_decode(self, startprob, means, covars, transmat):
        """Viterbi states (T int32)."""
        sp = np.ascontiguousarray(startprob, dtype=np.float64)
        mu = np.ascontiguousarray(means, dtype=np.float64)
        cv = np.ascontiguousarray(covars, dtype=np.float64)
        tm = np.ascontiguousarray(transmat, dtype=np.float64)
        out = np.empty(self._hmm_shape[0], np.int32)
        _check(self._lib.hicmi_hmm_decode(self._h, _ptr(sp), _ptr(mu), _ptr(cv), _ptr(tm), _ptr(out)))
        return out

    HMM_MAX_SLOTS = 16                                     # HICMI_HMM_MAX_SLOTS
    HMM_MAX_PROBLEMS = 256                                 # HICMI_HMM_MAX_PROBLEMS: larger batches go in chunks

    def hmm_load_obs_slot(self, slot, order, c, p):
        """hmm_load_obs into observation slot ``slot`` (the selected slot does not change unless it is this one).
        Returns (T, D)."""
        order = np.ascontiguousarray(order, dtype=np.int32)
        _check(self._lib.hicmi_hmm_load_obs_slot(self._h, int(slot), _ptr(order), len(order), int(c), int(p)))
        shapes = self.__dict__.setdefault("_hmm_slots", {})
        shapes[int(slot)] = [len(order) - int(c), int(p) - int(c), int(p) - int(c)]
        if int(slot) == getattr(self, "_hmm_cur", 0):
            self._hmm_shape = shapes[int(slot)]
        return len(order) - int(c), int(p) - int(c)

    def hmm_use_obs(self, slot):
        """Make slot ``slot`` the X of the single-problem hmm_* calls."""
        _check(self._lib.hicmi_hmm_use_obs(self._h, int(slot)))
        self._hmm_cur = int(slot)
        self._hmm_shape = self._hmm_slots[int(slot)]

    def hmm_slot_rows(self, slot):
        return self._hmm_slots[int(slot)][0]

    def hmm_dist2_multi(self, problems):
        """hmm_dist2 of many views at once: ``problems`` = [(slot, width, rows)] with 1 or 2 rows each; returns one
        len(rows) x T array per problem."""
        out = []
        for c0 in range(0, len(problems), self.HMM_MAX_PROBLEMS):
            part = problems[c0:c0 + self.HMM_MAX_PROBLEMS]
            k = len(part)
            slots = np.array([int(q[0]) for q in part], np.int64)
            widths = np.array([int(q[1]) for q in part], np.int64)
            nrows = np.array([len(q[2]) for q in part], np.int64)
            rows = np.zeros(2 * k, np.int64)
            for j, q in enumerate(part):
                rows[2 * j:2 * j + len(q[2])] = [int(r) for r in q[2]]
            Ts = [self.hmm_slot_rows(s) for s in slots]
            buf = np.empty(int(sum(int(r) * T for r, T in zip(nrows, Ts))), np.float64)
            _check(self._lib.hicmi_hmm_dist2_multi(self._h, k, _ptr(slots), _ptr(widths), _ptr(nrows), _ptr(rows),
                                                   _ptr(buf)))
            off = 0
            for r, T in zip(nrows, Ts):
                out.append(buf[off:off + int(r) * T].reshape(int(r), T))
                off += int(r) * T
        return out

    def hmm_kmeans_multi(self, problems):
        """hmm_kmeans of many views in lock step: ``problems`` = [(slot, width, (row0, row1), max_iter, tol)], the
        initial centers being those rows of the view; returns [(centers 2 x width, inertia, iterations)]."""
        out = []
        for c0 in range(0, len(problems), self.HMM_MAX_PROBLEMS):
            part = problems[c0:c0 + self.HMM_MAX_PROBLEMS]
            k = len(part)
            slots = np.array([int(q[0]) for q in part], np.int64)
            widths = np.array([int(q[1]) for q in part], np.int64)
            rows = np.array([int(r) for q in part for r in q[2]], np.int64)
            max_iter = np.array([int(q[3]) for q in part], np.int64)
            tol = np.array([float(q[4]) for q in part], np.float64)
            cen = np.empty(int(2 * widths.sum()), np.float64)
            inertia = np.empty(k, np.float64)
            n_iter = np.empty(k, np.int64)
            _check(self._lib.hicmi_hmm_kmeans_multi(self._h, k, _ptr(slots), _ptr(widths), _ptr(rows), _ptr(max_iter),
                                                    _ptr(tol), _ptr(cen), _ptr(inertia), _ptr(n_iter)))
            off = 0
            for j, D in enumerate(widths):
                out.append((cen[off:off + 2 * int(D)].reshape(2, int(D)), float(inertia[j]), int(n_iter[j])))
                off += 2 * int(D)
        return out

    # ---- Louvain tail (modularity > 0, S2C:239-349)
    def louvain_graph(self, rows):
        """A = graph_weights(log_transform(similarity of ``rows`` x ``rows``)) built on the device; returns m."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        self._lv_m = 0
        _check(self._lib.hicmi_louvain_graph(self._h, _ptr(rows), len(rows)))
        self._lv_m = len(rows)
        return self._lv_m

    def louvain_set_graph(self, A):
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != A.shape[1]:
            raise ValueError("A must be square")
        self._lv_m = 0
        _check(self._lib.hicmi_louvain_set_graph(self._h, _ptr(A), A.shape[0]))
        self._lv_m = A.shape[0]

    def louvain_get_graph(self, with_matrix=True):
        """(A or None, gdegrees, total_weight) of the graph on the device."""
        m = self._lv_m
        A = np.empty((m, m), np.float64) if with_matrix else None
        gdeg, tw = np.empty(m, np.float64), np.empty(1, np.float64)
        _check(self._lib.hicmi_louvain_get_graph(self._h, _ptr(A), _ptr(gdeg), _ptr(tw)))
        return A, gdeg, float(tw[0])

    def louvain_level0(self, states):
        """Level 0 of best_partition for every PCG64 state in ``states`` (rng.bit_generator.state dicts).  Returns
        (node2com R x m, states after, info R x 4 [passes, tie replays, near-threshold passes, 0], degrees R x m,
        internals R x m)."""
        R, m = len(states), self._lv_m
        st = np.empty((R, 6), np.uint64)
        for r, d in enumerate(states):
            s, inc = int(d["state"]["state"]), int(d["state"]["inc"])
            st[r] = [s & _M64, s >> 64, inc & _M64, inc >> 64, int(d["has_uint32"]), int(d["uinteger"])]
        n2c, st_out = np.empty((R, m), np.int32), np.empty((R, 6), np.uint64)
        info = np.empty((R, 4), np.int32)
        deg, inr = np.empty((R, m), np.float64), np.empty((R, m), np.float64)
        _check(self._lib.hicmi_louvain_level0(self._h, R, _ptr(st), _ptr(n2c), _ptr(st_out), _ptr(info), _ptr(deg),
                                              _ptr(inr)))
        out = []
        for r in range(R):
            v = [int(x) for x in st_out[r]]
            out.append({"bit_generator": "PCG64", "state": {"state": v[0] | (v[1] << 64), "inc": v[2] | (v[3] << 64)},
                        "has_uint32": v[4], "uinteger": v[5]})
        return n2c, out, info, deg, inr

    def louvain_induced(self, part, k):
        """modularity._induced(A, part): k x k."""
        part = np.ascontiguousarray(part, dtype=np.int32)
        out = np.empty((int(k), int(k)), np.float64)
        _check(self._lib.hicmi_louvain_induced(self._h, _ptr(part), len(part), int(k), _ptr(out)))
        return out

    def louvain_modularity(self, parts):
        """modularity.modularity(part, A) of every row of ``parts`` (R x m)."""
        parts = np.ascontiguousarray(np.atleast_2d(parts), dtype=np.int32)
        q = np.empty(parts.shape[0], np.float64)
        _check(self._lib.hicmi_louvain_modularity(self._h, _ptr(parts), parts.shape[0], parts.shape[1], _ptr(q)))
        return q

    # ---- misc
    def synchronize(self):
        _check(self._lib.hicmi_synchronize(self._h))

    def stream(self) -> int:
        s = _vp()
        _check(self._lib.hicmi_stream(self._h, ctypes.byref(s)))
        return s.value or 0

    def timing_enable(self, on=True):
        """True / 1: HIP events around every kernel family; 2: only around the few-launch Part 1 families
        (hicmi.h); False / 0: off."""
        _check(self._lib.hicmi_timing_enable(self._h, int(on)))
        for w in self._workers:
            w.timing_enable(on)

    def timing_reset(self):
        _check(self._lib.hicmi_timing_reset(self._h))
        for w in self._workers:
            w.timing_reset()

    def timing(self):
        """Per kernel family: device ms, launches, algorithmic bytes - summed over this context and
        the worker contexts that share its matrix."""
        out = self._timing_one()
        for w in self._workers:
            for k, v in w._timing_one().items():
                for f in ("ms", "launches", "bytes"):
                    out[k][f] += v[f]
        return out

    def _timing_one(self):
        names = ctypes.create_string_buffer(1024)
        ms = np.zeros(32, np.float64)
        launches = np.zeros(32, np.int64)
        nbytes = np.zeros(32, np.float64)
        cnt = c_i64()
        _check(self._lib.hicmi_timing_get(self._h, names, 1024, _ptr(ms), _ptr(launches), _ptr(nbytes), 32,
                                          ctypes.byref(cnt)))
        out = {}
        for k, nm in enumerate(names.value.decode().split(";")[:cnt.value]):
            out[nm] = dict(ms=float(ms[k]), launches=int(launches[k]), bytes=float(nbytes[k]))
        return out
