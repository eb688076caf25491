"""Row shards (hicmi_set_row_shard) held to the unsharded oracle.

After ``set_row_shard(first, stride)`` a context answers four stages only for the rows first, first + stride, ... : the
row sums, the per-row sort with its rank rows, the cut scan and the filter scan.  The functions here take a context-like
object (``_lib.Context`` on the device, ``fake_context.OracleContext`` on the CPU), drive the product's own sequence for
every ``first`` of a stride on ONE context - emulating every rank of a ``stride``-GPU run in turn -

    set_contacts -> set_row_shard(first, stride) -> row_sums() -> [the vectors of all firsts, gathered]
                 -> set_row_sums(full) -> upgma() -> rank_matrix(order) -> cut_scan / filter_scan

and compare what the context owns with ``Reference``: the oracle's row sums, rank rows, counts and SciPy decisions of
the WHOLE map, computed from the contact matrix alone and never from the library.  Every quantity is an integer, a bit
pattern or a flag, so every comparison is an equality."""
import numpy as np

import hic_oracle as orc

EINVAL = -1                                             # HICMI_EINVAL (include/hicmi.h)
NOT_RANKED = "hicmi_rank_matrix has not run"
WHOLE_MATRIX = "need the whole rank matrix (no row shard)"
BAD_SHARD = "row shard needs 0 <= first < stride"
COMPARED = {"row sums": 0, "rank rows": 0, "cut scans": 0, "filter scans": 0}      # how much the checks have looked at


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Reference:
    """The whole-map answers for contact matrix ``c`` sorted in ``order`` (default: the oracle's own leaf order).
    ``full=False`` keeps the rank rows per row (for maps too wide to argsort whole in a test); the scans need ``full``."""

    def __init__(self, c, order=None, full=True):
        self.c = np.ascontiguousarray(c, dtype=np.float64)
        self.n = n = len(self.c)
        self.np_sum, self.seq_sum = orc.np_row_sums(self.c), orc.seq_row_sums(self.c)
        assert np.all(self.np_sum != 0), "a map with empty rows is compacted before these stages"
        if order is None:
            order, _z = orc.average_cluster_leaves(orc.to_distance(self.c))
            self.order_is_leaves = True
        else:
            self.order_is_leaves = False
        self.order = np.asarray(order, dtype=np.int64)
        assert np.array_equal(np.sort(self.order), np.arange(n))
        self.sim = self.R = None
        if full:
            # the similarity of the reordered map and its rank order, as _oracle_rank of tests/test_gpu_parity.py forms them
            bins = [orc.Bin(i, "s", 0, 0, 0.0, 0.0) for i in range(n)]
            mat, bins = orc.remove_zero_rows(self.c.copy(), bins)
            dist = orc.to_distance(mat)[:, self.order][self.order]
            self.sim = orc.to_similarity(dist, [bins[i] for i in self.order])
            self.R = orc.rank_order(self.sim)
        self._x, self._sig = {}, {}

    def sim_row(self, a):
        """Row ``a`` of the reordered similarity: the same three roundings per cell as the whole-matrix expression."""
        if self.sim is not None:
            return self.sim[a]
        pa = self.order[a]
        dist = (1.0 - (self.c[pa] / self.np_sum[pa])) + 1.0
        return self.seq_sum[pa] * (1.0 - (dist[self.order] - 1.0))

    def rank_row(self, a):
        """Columns of row ``a`` by descending similarity, equal values by descending column."""
        if self.R is not None:
            return self.R[a]
        return np.argsort(self.sim_row(a), kind="stable")[::-1]

    def rank_row_inverse(self, a):
        inv = np.empty(self.n, dtype=np.int64)
        inv[self.rank_row(a)] = np.arange(self.n)
        return inv

    def tied_rows(self):
        """Rows (positions in ``order``) whose similarity row holds two equal values."""
        return [a for a in range(self.n) if len(np.unique(self.sim_row(a))) < self.n]

    # ---- the scans, from R alone
    def cut_x(self, start):
        if start not in self._x:
            self._x[start] = orc.first_pass_counts(self.R, start)[start:]
        return self._x[start]

    def cut_sig(self, start, M, psig):
        """S2C:455-469 as test_cut_and_filter_scans_match_oracle decides: sf(x - 1, M, L, L) >= psig -> 0, NaN -> 1,
        entry 0 -> 0."""
        from scipy.stats import hypergeom
        key = (start, M, psig)
        if key not in self._sig:
            x = self.cut_x(start)
            L = np.arange(1, self.n - start)
            with np.errstate(all="ignore"):
                p = hypergeom.sf(x[1:] - 1, M, L, L)
            self._sig[key] = np.concatenate(([0], np.where(p >= psig, 0, 1)))
        return self._sig[key]

    def filter_x(self, start, cut, n_rows):
        sub = self.R[start:start + n_rows, :cut - start]
        return np.count_nonzero((sub >= start) & (sub <= cut), axis=1)

    def filter_sig(self, start, cut, n_rows, M, psig):
        """S2C:631-636: sf(x - 1, M, L, L) < psig -> 1 with L = cut - start, NaN -> 0."""
        from scipy.stats import hypergeom
        with np.errstate(all="ignore"):
            p = hypergeom.sf(self.filter_x(start, cut, n_rows) - 1, M, cut - start, cut - start)
        return np.where(p < psig, 1, 0)


# ------------------------------------------------------------------------------------------------ the maps
def tie_free_map(n, seed):
    """The map of test_rank_matrix_bit_exact: no two contacts of a row are equal."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, n)) + 0.01
    return c + c.T


def quantised_map(n, seed):
    """The map of test_rank_matrix_tie_rule: integers 0..4, every row is a handful of long runs of equal values."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 5, size=(n, n)).astype(np.float64)
    return np.triu(c, 1) + np.triu(c, 1).T + np.eye(n) * 3


def planted_map(n, seed, n_rows=40):
    """Ties planted as in test_rank_rows_with_short_runs_of_equal_similarities, in ``n_rows`` rows of a tie-free map:
    three runs of 2 .. 8 equal values each at random sorted positions, a run of 9 in every tenth row and one of 13 in
    another tenth (rows the short-run kernel must leave to the full network).  Returns (map, the planted rows)."""
    rng = np.random.default_rng(seed)
    c = rng.random((n, n)) + 0.01
    c = np.triu(c) + np.triu(c, 1).T
    rows = rng.choice(n, size=n_rows, replace=False)
    for t, r in enumerate(rows):
        by_value = np.argsort(c[r], kind="stable")
        lengths = [2 + (t % 7)] * 3
        if t % 10 == 3:
            lengths += [9]
        if t % 10 == 7:
            lengths = [13] + lengths
        for L in lengths:
            p0 = int(rng.integers(0, n - L))
            cols = by_value[p0:p0 + L]
            c[r, cols] = c[r, cols[0]]
            c[cols, r] = c[r, cols[0]]
    return c, [int(r) for r in rows]


# ------------------------------------------------------------------------------------------------ the cases of a scan
def scan_starts(n, stride):
    """0 .. stride + 1 and the far end: every residue of (first - start) mod stride occurs for every first."""
    want = list(range(stride + 2)) + [n // 3, n - stride - 1, n - 2, n - 1]
    return sorted({s for s in want if 0 <= s < n})


def scan_Ms(n, start):
    """Two different M per start, the second answered from the cached counts: the whole tail, and 3 (2 where the tail is 3)."""
    return [n - start, 3 if n - start != 3 else 2]


def filter_triples(n, stride, seed=5):
    """(start, cut, n_rows): no row, one row (own for one first, foreign for the others), fewer rows than the distance to
    the first own row (for the firsts further away), cut == start, cut == n - 1, and a dozen random ones."""
    out = []
    for s in range(min(stride, n)):                                            # one and two rows at every residue
        out += [(s, min(n - 1, s + 5), k) for k in (1, 2) if k <= n - s]
    for s in sorted(v for v in {0, 1, n // 3} if v < n):
        far = min(n - 1, s + max(2, (n - s) // 2))
        room = n - s
        for n_rows in sorted({0, 1, 2, stride - 1, stride, stride + 1, room}):
            if n_rows <= room:
                out.append((s, far, n_rows))
        out.append((s, s, min(room, stride + 1)))                              # cut == start: L = 0
        out.append((s, n - 1, min(room, 2 * stride + 1)))
    rng = np.random.default_rng(seed)
    for _ in range(12 if n > 3 else 0):
        start = int(rng.integers(0, n - 2))
        cut = int(rng.integers(start, n))
        out.append((start, cut, int(rng.integers(1, n - start + 1))))
    return out


# ------------------------------------------------------------------------------------------------ refusals
def refused(call, text, code=EINVAL):
    """``call()`` must be refused with libhicmi's error ``code`` and a message holding ``text``."""
    try:
        call()
    except RuntimeError as e:                                                  # _lib.HicmiError / fake_context.OracleError
        assert ("error %d:" % code) in str(e) and text in str(e), "refused, but with: %s" % e
        return
    raise AssertionError("the call was answered; it should have been refused with '%s'" % text)


# ------------------------------------------------------------------------------------------------ the stages
def own_mask(n, first, stride, row0=0):
    return (np.arange(row0, n) % stride) == first


def check_row_sums(ctx, ref, stride, load):
    """The shard sums of every first on one upload; returns the gathered (full) vectors."""
    n = ref.n
    load(ctx)
    total_np, total_seq = np.zeros(n), np.zeros(n)
    for first in range(stride):
        ctx.set_row_shard(first, stride)
        a, b = ctx.row_sums()
        own = own_mask(n, first, stride)
        assert same_bits(a[own], ref.np_sum[own]) and same_bits(b[own], ref.seq_sum[own]), (first, stride)
        assert same_bits(a[~own], np.zeros(n - own.sum())) and same_bits(b[~own], np.zeros(n - own.sum())), (first, stride)
        total_np += a
        total_seq += b
        COMPARED["row sums"] += 1
    assert same_bits(total_np, ref.np_sum) and same_bits(total_seq, ref.seq_sum), stride
    return total_np, total_seq


def check_rank_rows(ctx, ref, first, stride, rows=None):
    """Own rows (all of them, or those of ``rows``) against the oracle's; no other row is read."""
    n = ref.n
    own = [a for a in range(first, n, stride) if rows is None or a in rows]
    for a in own:
        inv = ctx.rank_rows(a, 1, inverse=True)
        assert inv.shape == (1, n) and np.array_equal(inv[0].astype(np.int64), ref.rank_row_inverse(a)), (first, stride, a)
        assert np.array_equal(ctx.rank_rows(a, 1)[0].astype(np.int64), ref.rank_row(a)), (first, stride, a)
    COMPARED["rank rows"] += len(own)
    return len(own)


def check_cut_scans(ctx, ref, first, stride, starts, psig=0.05):
    n = ref.n
    for start in starts:
        own = own_mask(n, first, stride, start)
        x_o = np.where(own, ref.cut_x(start), 0)
        for M in scan_Ms(n, start):                                # (the second M: counts cached by the first)
            what = (first, stride, start, M)
            sig_o = np.where(own, ref.cut_sig(start, M, psig), 0)
            sig, x = ctx.cut_scan(start, M, psig, want_x=True)
            assert x.shape == (n - start,) and np.array_equal(x, x_o), what
            assert np.array_equal(sig, sig_o), what
            assert np.array_equal(ctx.cut_scan(start, M, psig), sig_o), what       # flags only: the pinned-buffer path
            COMPARED["cut scans"] += 2


def check_filter_scans(ctx, ref, first, stride, triples, psig=0.01):
    n = ref.n
    for start, cut, n_rows in triples:
        own = own_mask(start + n_rows, first, stride, start)
        x_o = np.where(own, ref.filter_x(start, cut, n_rows), 0)
        for M in scan_Ms(n, start):
            what = (first, stride, start, cut, n_rows, M)
            sig_o = np.where(own, ref.filter_sig(start, cut, n_rows, M, psig), 0)
            sig, x = ctx.filter_scan(start, cut, n_rows, M, psig, want_x=True)
            assert x.shape == (n_rows,) and np.array_equal(x, x_o), what
            assert np.array_equal(sig, sig_o), what
            assert np.array_equal(ctx.filter_scan(start, cut, n_rows, M, psig), sig_o), what
            COMPARED["filter scans"] += 2


def check_stride(ctx, ref, stride, firsts=None, upgma=False, rows=None, starts=None, triples=None, load=None,
                 reload_each=True, after_rank=None):
    """Every ``first`` of ``stride`` (or those of ``firsts``) on ``ctx``, stage by stage.  ``upgma``: cluster before the
    sort (the order must then be the oracle's leaves); ``starts`` / ``triples``: the scans to run (None: none; they need a
    full reference); ``load``: how the matrix reaches the context (default set_contacts); ``after_rank(ctx, first)``: the
    caller's look at the context after every rank_matrix.  Returns the number of rank rows compared."""
    assert stride > 1, "a stride of 1 is no shard"
    load = load or (lambda c: c.set_contacts(ref.c))
    full = check_row_sums(ctx, ref, stride, load)
    compared = 0
    for k, first in enumerate(range(stride) if firsts is None else firsts):
        if reload_each or k == 0:
            load(ctx)
        ctx.set_row_shard(first, stride)
        ctx.set_row_sums(*full)
        a, b = ctx.row_sums()                                       # installed: the complete vectors, unchanged
        assert same_bits(a, ref.np_sum) and same_bits(b, ref.seq_sum), (first, stride)
        if upgma:
            assert ref.order_is_leaves
            leaves, _z = ctx.upgma(want_linkage=False)
            assert np.array_equal(leaves, ref.order), (first, stride)
        ctx.rank_matrix(ref.order)
        if after_rank is not None:
            after_rank(ctx, first)
        compared += check_rank_rows(ctx, ref, first, stride, rows)
        if starts is not None:
            check_cut_scans(ctx, ref, first, stride, starts)
        if triples is not None:
            check_filter_scans(ctx, ref, first, stride, triples)
    return compared


def check_whole(ctx, ref, starts, triples):
    """set_row_shard(0, 1) on a context that was sharded: whole-matrix answers again, all equal to the oracle."""
    n = ref.n
    ctx.set_row_shard(0, 1)
    refused(lambda: ctx.rank_rows(0, 1), NOT_RANKED)
    a, b = ctx.row_sums()
    assert same_bits(a, ref.np_sum) and same_bits(b, ref.seq_sum)
    ctx.rank_matrix(ref.order)
    assert np.array_equal(ctx.rank_rows().astype(np.int64), np.stack([ref.rank_row(r) for r in range(n)]))
    assert np.array_equal(ctx.rank_rows(inverse=True).astype(np.int64), np.stack([ref.rank_row_inverse(r) for r in range(n)]))
    for start in starts:
        for M in scan_Ms(n, start):
            sig, x = ctx.cut_scan(start, M, 0.05, want_x=True)
            assert np.array_equal(x, ref.cut_x(start)) and np.array_equal(sig, ref.cut_sig(start, M, 0.05)), (start, M)
            assert np.array_equal(ctx.cut_scan(start, M, 0.05), sig), (start, M)
    for start, cut, n_rows in triples:
        M = n - start
        sig, x = ctx.filter_scan(start, cut, n_rows, M, 0.01, want_x=True)
        assert np.array_equal(x, ref.filter_x(start, cut, n_rows)), (start, cut, n_rows)
        assert np.array_equal(sig, ref.filter_sig(start, cut, n_rows, M, 0.01)), (start, cut, n_rows)


def check_state_rules(ctx, ref, stride):
    """What a context refuses around a shard, for every ``first`` on this one context, and the way back to the whole
    matrix.  Needs n >= 2."""
    assert stride > 1 and ref.n >= 2
    n = ref.n
    starts, triples = scan_starts(n, stride), filter_triples(n, stride)
    ctx.set_contacts(ref.c)
    ctx.set_row_shard(0, 1)
    ctx.set_row_sums(ref.np_sum, ref.seq_sum)
    ctx.rank_matrix(ref.order)
    ctx.cut_scan(0, n, 0.05)                                         # ranked: answered
    for first in range(stride):
        ctx.set_row_shard(first, stride)
        assert ctx.shard == (first, stride)
        # the rank rows and counts in the context are another shard's: nothing reads them before the next rank_matrix
        refused(lambda: ctx.cut_scan(0, n, 0.05), NOT_RANKED)
        refused(lambda: ctx.cut_scan(0, n, 0.05, want_x=True), NOT_RANKED)
        refused(lambda: ctx.filter_scan(0, n - 1, 1, n, 0.05), NOT_RANKED)
        refused(lambda: ctx.rank_rows(first % n, 1), NOT_RANKED)
        refused(lambda: ctx.rank_rows(first % n, 1, inverse=True), NOT_RANKED)
        ctx.rank_matrix(ref.order)
        # the scan loops on the device walk every row
        refused(lambda: ctx.first_pass_cuts(2, n, 0.05), WHOLE_MATRIX)
        refused(lambda: ctx.filter_cuts([1], 0.05), WHOLE_MATRIX)
        # a shard that is none: refused, and (first, stride) stays in force with its rank rows
        for bad in ((stride, stride), (-1, stride), (0, 0)):
            refused(lambda: ctx.set_row_shard(*bad), BAD_SHARD)
            assert ctx.shard == (first, stride)
        check_rank_rows(ctx, ref, first, stride)
        check_cut_scans(ctx, ref, first, stride, starts[:3] + starts[-2:])
        check_filter_scans(ctx, ref, first, stride, triples[:6])
    check_whole(ctx, ref, starts, triples)
