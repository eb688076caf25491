"""Row shards of every stride and offset on the device (run with -m gpu on an MI355X).

tests/shard_reference.py emulates every rank of a 2-, 3- and 8-GPU run in turn on one context: set the shard, run the
stage, compare what the context owns with the unsharded oracle - row sums bit for bit, rank rows, counts and flags as
integers - for every ``first``.  The sizes are the smallest at which each path exists: widths below the stride, the
per-call sorters (register-blocked network, LSD radix, LDS network) with and without ties, a row of two radix tiles,
the rows sorted beside the nn-chain and re-addressed or finished by the tied-row kernels, an adopted matrix with
ld > n, and scans whose start, range and cached counts fall every way against the shard."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import adopted_matrix as am
import golden_cases as gc
import shard_reference as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDES = [2, 3, 8]
SORT_SWITCHES = ("HICMI_SORT_LDS", "HICMI_SORT_RADIX", "HICMI_NO_PRESORT", "HICMI_PRESORT_FROM", "HICMI_PRESORT_TIES",
                 "HICMI_TEST_PRESORT_ALL_LEAVE")


@pytest.fixture(scope="module")
def hic():
    from hic_genome_assembler_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    """When this file's first test started and what the checker had compared by then (the last test reports both)."""
    return time.perf_counter(), dict(sr.COMPARED)


@pytest.fixture
def plain_sort(monkeypatch):
    for name in SORT_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


# ------------------------------------------------------------------------------------------------ the maps
@functools.lru_cache(maxsize=None)
def _per_call(kind, n):
    """A map sorted in a random order, never clustered: every hicmi_rank_matrix sorts its rows itself."""
    order = np.random.default_rng(n + 1).permutation(n)
    if kind == "tie-free":
        return sr.Reference(sr.tie_free_map(n, n), order)
    ref = sr.Reference(sr.quantised_map(n, 21), order)
    assert all(len(np.unique(ref.sim[a])) < n // 10 for a in range(n))            # every row is tied, heavily
    return ref


@functools.lru_cache(maxsize=None)
def _clustered(kind):
    """A 600-bin map sorted in its own leaf order: (reference, planted rows as positions of the order, tied positions)."""
    n = 600
    planted = []
    if kind == "tie-free":
        c = sr.tie_free_map(n, 600)
    elif kind == "planted":
        c, planted = sr.planted_map(n, 601)
    else:
        c = sr.quantised_map(n, 602)
    ref = sr.Reference(c)
    where = {int(r): a for a, r in enumerate(ref.order)}
    planted = sorted(where[r] for r in planted)
    tied = ref.tied_rows()
    assert set(planted) <= set(tied)
    if kind == "tie-free":
        assert tied == []
    elif kind == "planted":
        assert len(planted) == 40 and len(tied) <= len(planted) + 3 + n // 400
        for stride in (3, 8):                                    # own rows and foreign rows among the tied, for any first
            assert len({a % stride for a in planted}) >= 2
    else:
        assert len(tied) == n
    return ref, planted, tied


@functools.lru_cache(maxsize=None)
def _golden(name):
    return sr.Reference(gc.load_case(name)[4])


def _not_presorted(ctx, first):
    assert ctx.presort_state() == (0, 0)


# ------------------------------------------------------------------------------------------------ widths below the stride
@pytest.mark.parametrize("n", [1, 2, 5, 9])
def test_widths_below_and_just_above_the_stride(hic, plain_sort, n):
    """Stride 8 on 1, 2, 5 and 9 rows: the ranks beyond the last row own nothing - sums and scans of zeros, a rank_matrix
    that succeeds - one rank owns two rows at n = 9, and no launch of an empty shard leaves an error behind: the whole
    matrix is answered on the same context afterwards."""
    ref = sr.Reference(sr.tie_free_map(n, n), np.random.default_rng(n).permutation(n))
    triples = sr.filter_triples(n, 8)
    with hic.Context(0) as ctx:
        assert sr.check_stride(ctx, ref, 8, starts=list(range(n)), triples=triples, after_rank=_not_presorted) == n
        sr.check_whole(ctx, ref, list(range(n)), triples)
        for stride in (2, 3):
            sr.check_stride(ctx, ref, stride, starts=list(range(n)), triples=triples)
        sr.check_whole(ctx, ref, list(range(n)), triples)


# ------------------------------------------------------------------------------------------------ the per-call sorters
def _per_call_case(ctx, kind, n, stride, load=None):
    ref = _per_call(kind, n)
    starts = sr.scan_starts(n, stride)[:4] if n < 300 else None
    assert sr.check_stride(ctx, ref, stride, starts=starts, load=load, after_rank=_not_presorted) == n


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("kind", ["tie-free", "quantised"])
def test_per_call_sorters(hic, plain_sort, kind, n, stride):
    """The register-blocked network (k_sort_rows_rb + k_rank_invert) and HICMI_SORT_RADIX=1 (k_sort_rows_radix), which
    are read per call: every first of the stride, every own row."""
    with hic.Context(0) as ctx:
        _per_call_case(ctx, kind, n, stride)
        plain_sort.setenv("HICMI_SORT_RADIX", "1")
        _per_call_case(ctx, kind, n, stride)


CHILD = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_shard as t; t.child_main()"
         % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))


def child_main():
    """HICMI_SORT_LDS is read once per process: the cases of test_per_call_sorters in a fresh child with the switch set."""
    from hic_genome_assembler_amd import _lib
    assert os.environ.get("HICMI_SORT_LDS")
    done = 0
    for kind in ("tie-free", "quantised"):
        for n in (257, 1000):
            for stride in STRIDES:
                with _lib.Context(0) as ctx:
                    _per_call_case(ctx, kind, n, stride)
                done += 1
    print("lds sorter under a shard: %d cases equal the oracle" % done)


def test_lds_sorter_in_a_fresh_process():
    env = {k: v for k, v in os.environ.items() if k not in SORT_SWITCHES}
    env["HICMI_SORT_LDS"] = "1"
    res = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "lds sorter under a shard: 12 cases equal the oracle" in res.stdout


def test_one_row_of_two_radix_tiles(hic, plain_sort):
    """n = 8193 under HICMI_SORT_RADIX=1: the shortest row that spans two 8192-element tiles, with 40 distinct contacts
    (ties across the tile boundary), as ranks 0 and 7 of 8 - the first, the middle and the last row each of them owns."""
    n = 8193
    rng = np.random.default_rng(8193)
    c = rng.integers(0, 40, size=(n, n)).astype(np.float64)      # (the sort reads rows: the map need not be symmetric)
    ref = sr.Reference(c, rng.permutation(n), full=False)
    rows = set()
    for first in (0, 7):
        own = list(range(first, n, 8))
        rows |= {own[0], own[len(own) // 2], own[-1]}
    assert len(rows) == 6 and {0, 7, 8191, 8192} <= rows          # 8192 = 0 mod 8, 8191 = 7 mod 8
    for a in sorted(rows):
        assert len(np.unique(ref.sim_row(a))) < n // 10
    plain_sort.setenv("HICMI_SORT_RADIX", "1")
    with hic.Context(0) as ctx:
        got = sr.check_stride(ctx, ref, 8, firsts=[0, 7], rows=rows, reload_each=False, after_rank=_not_presorted)
    assert got == 6


# ------------------------------------------------------------------------------------------------ rows sorted beside the chain
def _presorted_case(hic, kind, stride):
    ref, planted, tied = _clustered(kind)
    n = ref.n

    def after_rank(ctx, first):
        state, n_tied = ctx.presort_state()
        assert state == 1
        if kind == "quantised":
            assert n_tied == n
        else:
            # (two close contacts can round to the same similarity: a few more rows than the planted ones may be flagged)
            assert len(planted) <= n_tied <= len(planted) + 3 + n // 400
        assert n_tied == len(tied)                               # the keys are the reference's similarities, bit for bit

    with hic.Context(0) as ctx:
        got = sr.check_stride(ctx, ref, stride, upgma=True, starts=sr.scan_starts(n, stride),
                              triples=sr.filter_triples(n, stride), after_rank=after_rank)
    assert got == n


@pytest.mark.parametrize("stride", [3, 8])
@pytest.mark.parametrize("kind", ["tie-free", "planted", "quantised"])
def test_rows_sorted_beside_the_chain_under_a_shard(hic, plain_sort, kind, stride):
    """HICMI_PRESORT_FROM=200 at 600 bins, leaves as the order: every rank pre-sorts ALL rows beside its chain and then
    re-addresses its own (k_rank_relabel), finishing its own tied rows with k_rank_rows_short_runs / k_rank_rows_tied
    through the own-row list - rows of other ranks are left alone.  Then every cut and filter scan of the clustered map."""
    plain_sort.setenv("HICMI_PRESORT_FROM", "200")
    _presorted_case(hic, kind, stride)


def test_tied_rows_sorted_again_in_full_under_a_shard(hic, plain_sort):
    """HICMI_PRESORT_TIES=resort: the own tied rows go through k_sort_rows_rb's row-list form and k_rank_invert's."""
    plain_sort.setenv("HICMI_PRESORT_FROM", "200")
    plain_sort.setenv("HICMI_PRESORT_TIES", "resort")
    _presorted_case(hic, "planted", 3)


# ------------------------------------------------------------------------------------------------ an adopted matrix
def test_adopted_matrix_under_a_shard(hic, plain_sort):
    """The per-call case n = 257, stride 3 on a torch tensor with ld = n + 3 handed over by set_contacts_device: distinct
    large finite values in the three padding cells of every row, and the storage keeps its bits."""
    import torch
    n, ld = 257, 260
    ref = _per_call("tie-free", n)
    store = torch.arange(n * ld, dtype=torch.float64, device="cuda:0") + am.FINITE_BASE
    view = store.view(n, ld)
    view[:, :n] = torch.as_tensor(ref.c, device="cuda:0")
    snapshot = store.view(torch.int64).clone()
    torch.cuda.synchronize()

    def load(ctx):
        ctx.set_contacts_device(view.data_ptr(), n, ld, keepalive=store)
        assert ctx.contacts_device() == (view.data_ptr(), n, ld)

    with hic.Context(0) as ctx:
        _per_call_case(ctx, "tie-free", n, 3, load=load)
        plain_sort.setenv("HICMI_SORT_RADIX", "1")
        _per_call_case(ctx, "tie-free", n, 3, load=load)
        am.assert_untouched(store, snapshot)


# ------------------------------------------------------------------------------------------------ scans of a golden map
@pytest.mark.parametrize("stride", STRIDES)
def test_scans_of_a_golden_map(hic, plain_sort, stride):
    """n160 clustered on the device, every start against the shard (all residues of (first - start) mod stride, the
    last rows), two M per start - the second from the cached counts - with and without the counts, and the filter
    triples of shard_reference.filter_triples."""
    ref = _golden("n160")
    with hic.Context(0) as ctx:
        got = sr.check_stride(ctx, ref, stride, upgma=True, starts=sr.scan_starts(ref.n, stride),
                              triples=sr.filter_triples(ref.n, stride), after_rank=_not_presorted)
    assert got == ref.n


# ------------------------------------------------------------------------------------------------ state rules
@pytest.mark.parametrize("stride", [3, 8])
def test_state_rules(hic, plain_sort, stride):
    """One context through every first: nothing is answered from another shard's rank rows, the device-driven scan loops
    are refused under a shard, a shard that is none is refused and changes nothing, and (0, 1) brings the whole matrix
    back."""
    with hic.Context(0) as ctx:
        sr.check_state_rules(ctx, _per_call("tie-free", 257), stride)


# ------------------------------------------------------------------------------------------------ the cost of this file
def test_wall_time_of_this_file_is_in_the_log(wall_time, capsys):
    """The last test of the file: the wall time since its first test, and how much the tests of this process compared
    with the oracle, printed past the capture (the LDS sorter's cases are compared in the child and are not counted).
    Run on its own it reports zeros."""
    t0, before = wall_time
    looked = {k: sr.COMPARED[k] - before[k] for k in sr.COMPARED}
    with capsys.disabled():
        print("\ntests/test_gpu_shard.py: %.1f s wall; compared with the oracle in this process: %s"
              % (time.perf_counter() - t0, ", ".join("%d %s" % (v, k) for k, v in looked.items())), flush=True)
    assert all(v >= 0 for v in looked.values())
