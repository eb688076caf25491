"""tests/shard_reference.py without a GPU: the checker and its references agree with the project's NumPy restatement of
the shard rules (fake_context.OracleContext) on the small maps of tests/test_gpu_shard.py, and the checker bites - three
stand-ins that get one shard rule wrong each are caught."""
import functools

import numpy as np
import pytest

import fake_context
import golden_cases as gc
import hic_oracle as orc
import shard_reference as sr

STRIDES = [2, 3, 8]


class ShardedOracle(fake_context.OracleContext):
    """OracleContext plus libhicmi's refusal of the device-driven scan loops under a shard (the oracle-backed context has
    no such loops: the host flow takes their absence for 'run the loops on the host')."""

    def first_pass_cuts(self, min_size, stop_ind, psig):
        if self.shard[1] != 1:
            raise fake_context.OracleError("libhicmi error -1: the device-driven scan loops need the whole rank matrix (no row shard)")
        raise NotImplementedError

    def filter_cuts(self, cuts, psig):
        if self.shard[1] != 1:
            raise fake_context.OracleError("libhicmi error -1: the device-driven scan loops need the whole rank matrix (no row shard)")
        raise NotImplementedError


@functools.lru_cache(maxsize=None)
def _reference(name):
    if name == "n160":
        return sr.Reference(gc.load_case("n160")[4])
    kind, n = name.split("-")
    n = int(n)
    order = np.random.default_rng(n + 1).permutation(n)
    if kind == "tiefree":
        return sr.Reference(sr.tie_free_map(n, n), order)
    if kind == "quantised":
        return sr.Reference(sr.quantised_map(n, 21), order)
    if kind == "planted":
        return sr.Reference(sr.planted_map(n, n, n_rows=12)[0])
    raise ValueError(name)


# ------------------------------------------------------------------------------------------------ the references
def test_reference_is_the_oracle_of_the_whole_map():
    """Row by row and whole, the reference is _oracle_rank of tests/test_gpu_parity.py and the scans' own oracle."""
    ref = _reference("tiefree-57")
    lazy = sr.Reference(ref.c, ref.order, full=False)
    for a in range(ref.n):
        assert sr.same_bits(lazy.sim_row(a), ref.sim[a])
        assert np.array_equal(lazy.rank_row(a), ref.R[a])
        assert np.array_equal(ref.rank_row_inverse(a)[ref.R[a]], np.arange(ref.n))
    with fake_context.OracleContext() as ctx:
        ctx.set_contacts(ref.c)
        ctx.rank_matrix(ref.order)
        assert np.array_equal(ctx.rank_rows().astype(np.int64), ref.R)
        for start in (0, 3, ref.n - 1):
            sig, x = ctx.cut_scan(start, ref.n - start, 0.05, want_x=True)
            assert np.array_equal(x, ref.cut_x(start)) and np.array_equal(sig, ref.cut_sig(start, ref.n - start, 0.05))


def test_the_tied_maps_are_tied():
    q = _reference("quantised-257")
    assert all(len(np.unique(q.sim[a])) < q.n // 10 for a in range(q.n))
    assert _reference("tiefree-257").tied_rows() == []
    c, rows = sr.planted_map(120, 120, n_rows=12)
    ref = sr.Reference(c)
    where = {int(r): a for a, r in enumerate(ref.order)}
    tied = ref.tied_rows()
    assert {where[r] for r in rows} <= set(tied) and len(tied) <= len(rows) + 3


def test_the_scan_cases_reach_every_residue_and_edge():
    for n, stride in ((160, 2), (160, 3), (600, 8), (9, 8)):
        starts = sr.scan_starts(n, stride)
        assert {0, n - 1} <= set(starts) and all(0 <= s < n for s in starts)
        for first in range(stride):
            assert {(first - s) % stride for s in starts} == set(range(stride))
        for start in starts:
            a, b = sr.scan_Ms(n, start)
            assert a != b and a == n - start
        triples = sr.filter_triples(n, stride)
        assert all(0 <= s <= c < n and 0 <= k <= n - s for s, c, k in triples)
        assert any(k == 0 for _s, _c, k in triples) and any(c == s for s, c, _k in triples)
        assert any(c == n - 1 for _s, c, _k in triples)
        for first in range(stride):
            t0 = [((first - s) % stride, k) for s, _c, k in triples]
            assert any(d == 0 and k == 1 for d, k in t0)                        # one row, an own one
            assert any(d > 0 and k == 1 for d, k in t0)                         # one row, a foreign one
            if stride > 2:
                assert any(1 < k <= d for d, k in t0)                           # rows, all before the first own one


# ------------------------------------------------------------------------------------------------ the checker, on the oracle
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n", [1, 2, 5, 9])
def test_degenerate_widths(n, stride):
    ref = sr.Reference(sr.tie_free_map(n, n), np.random.default_rng(n).permutation(n))
    triples = sr.filter_triples(n, stride)
    with ShardedOracle() as ctx:
        got = sr.check_stride(ctx, ref, stride, starts=list(range(n)), triples=triples)
        assert got == n
        sr.check_whole(ctx, ref, list(range(n)), triples)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", ["tiefree-257", "quantised-257"])
def test_random_order_maps(name, stride):
    ref = _reference(name)
    with ShardedOracle() as ctx:
        assert sr.check_stride(ctx, ref, stride, starts=sr.scan_starts(ref.n, stride)[:4]) == ref.n


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("name", ["n160", "planted-120"])
def test_clustered_maps_with_every_scan(name, stride):
    ref = _reference(name)
    with ShardedOracle() as ctx:
        got = sr.check_stride(ctx, ref, stride, upgma=True, starts=sr.scan_starts(ref.n, stride),
                              triples=sr.filter_triples(ref.n, stride))
        assert got == ref.n


@pytest.mark.parametrize("stride", [3, 8])
def test_state_rules(stride):
    with ShardedOracle() as ctx:
        sr.check_state_rules(ctx, _reference("tiefree-57"), stride)


# ------------------------------------------------------------------------------------------------ the checker bites
class OwnRowsCountedFromTheStart(ShardedOracle):
    """Takes entry t of a scan for its own when t % stride == first - right only where start is a multiple of the stride."""

    def _owned(self, first_row, count):
        first, stride = self.shard
        return (np.arange(count) % stride) == first


class ForeignCountsLeftIn(ShardedOracle):
    """The flags are masked, the counts of the other shards' rows are not."""

    def cut_scan(self, start, M, psig, want_x=False):
        out = super().cut_scan(start, M, psig, want_x)
        if not want_x:
            return out
        return out[0], orc.first_pass_counts(self.R, start)[start:].astype(np.int32)


class CachedFlagsOfTheFirstM(ShardedOracle):
    """Keeps the flags with the cached counts: a second M on the same start gets the first M's answer."""

    def rank_matrix(self, order):
        super().rank_matrix(order)
        self._cached = None

    def cut_scan(self, start, M, psig, want_x=False):
        if self._cached is None or self._cached[0] != start:
            self._cached = (start,) + super().cut_scan(start, M, psig, True)
        _s, sig, x = self._cached
        return (sig, x) if want_x else sig

    def filter_scan(self, *a, **kw):
        self._cached = None
        return super().filter_scan(*a, **kw)


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("wrong", [OwnRowsCountedFromTheStart, ForeignCountsLeftIn, CachedFlagsOfTheFirstM])
def test_a_wrong_shard_rule_is_caught(wrong, stride):
    ref = _reference("n160")
    starts, triples = sr.scan_starts(ref.n, stride), sr.filter_triples(ref.n, stride)
    with ShardedOracle() as ctx:                                               # the same call on the right stand-in passes
        sr.check_stride(ctx, ref, stride, firsts=[stride - 1], starts=starts, triples=triples)
    with wrong() as ctx:
        with pytest.raises(AssertionError):
            sr.check_stride(ctx, ref, stride, firsts=[stride - 1], starts=starts, triples=triples)


def test_a_missing_refusal_is_caught():
    class AnswersBeforeTheSort(ShardedOracle):
        def set_row_shard(self, first, stride):
            kept = self.R
            super().set_row_shard(first, stride)
            self.R = kept

    class TakesAnyShard(ShardedOracle):
        def set_row_shard(self, first, stride):
            self.shard = (int(first), int(stride))
            self.R = None

    for wrong in (AnswersBeforeTheSort, TakesAnyShard):
        with wrong() as ctx:
            with pytest.raises(AssertionError):
                sr.check_state_rules(ctx, _reference("tiefree-57"), 3)
