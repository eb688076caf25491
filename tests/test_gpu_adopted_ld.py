"""Every stage that reads the contact matrix, on a matrix adopted with hicmi_set_contacts_device whose rows are ld > n
doubles apart (tests/adopted_matrix.py: an odd ld, an even ld on a base that is not 16-byte aligned, wide padding, a
square block of a larger map).  Each stage is held to the reference its own test in this suite uses, at that test's
tolerance - bit for bit wherever that test is bit-exact - and, where stated, to the same call on a context that owns a
dense copy.  Everything outside the n x n cells is poison (NaN for single-pass stages, large distinct finite values for
stages that iterate or sort), and every test ends by checking that the adopted storage still holds its bits.

The stages with older ld tests (group sums, junction sums, ICE, rebin) are not repeated here."""
import contextlib
import ctypes
import functools
import hashlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import adopted_matrix as am
import golden_cases as gc
import hmm_reference as href

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = list(am.LAYOUTS)
EINVAL = -1                                             # HICMI_EINVAL (include/hicmi.h)


@pytest.fixture(scope="module")
def hic():
    from hic_genome_assembler_amd import _lib
    _lib.load()
    return _lib


@pytest.fixture(scope="module")
def orc():
    import hic_oracle
    return hic_oracle


def _quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **kw)


def _ulps(a, b):
    return np.abs(a.view(np.int64) - b.view(np.int64))


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------------- row sums
@functools.lru_cache(maxsize=2)
def _row_sum_case(n):
    """The matrix of test_row_sums_bit_exact (at most 300 non-zero rows) and the oracle's two sums of those rows."""
    import hic_oracle as orc
    rng = np.random.default_rng(n)
    rows = min(n, 300)
    m = np.zeros((n, n))
    m[:rows] = rng.random((rows, n)) * 1000.0
    return m, rows, orc.np_row_sums(m[:rows]), orc.seq_row_sums(m[:rows])


# 8: the first 16-byte body of k_row_sums_seq; 129: two leaves; 8200: a second 8192-element chunk
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 7, 8, 129, 2049, 8200])
def test_row_sums(hic, layout, n):
    m, rows, np_ref, seq_ref = _row_sum_case(n)
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, m, layout)
        np_sum, seq = ctx.row_sums()
        am.assert_untouched(store, snap)
    assert np.array_equal(np_sum[:rows], np_ref)
    assert np.array_equal(seq[:rows], seq_ref)
    assert np.all(np_sum[rows:] == 0) and np.all(seq[rows:] == 0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_sums_of_a_shard(hic, layout):
    """set_row_shard(1, 3): rows 1, 4, 7, ... are summed, the other entries read exactly 0."""
    n = 129
    m, rows, np_ref, seq_ref = _row_sum_case(n)
    own = np.arange(n) % 3 == 1
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, m, layout)
        ctx.set_row_shard(1, 3)
        np_sum, seq = ctx.row_sums()
        am.assert_untouched(store, snap)
    assert np.array_equal(np_sum[own], np_ref[own]) and np.array_equal(seq[own], seq_ref[own])
    assert np.all(np_sum[~own] == 0) and np.all(seq[~own] == 0)
    assert own.sum() == 43 and np.all(np_ref[own] != 0)


# --------------------------------------------------------------------------------- row fetch
def _fetch(ctx, row0, nrows, n):
    out = np.full((max(nrows, 1), n), -7.0)
    rc = ctx._lib.hicmi_get_contact_rows(ctx._h, int(row0), int(nrows), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_fetch(hic, layout):
    n = 600
    M = np.random.default_rng(31).random((n, n)) * 50.0
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, M, layout)
        assert _same_bits(ctx.contacts_host(), M)
        for row0, nrows in ((0, n), (5, 1), (n - 1, 1)):
            assert _same_bits(_fetch(ctx, row0, nrows, n), M[row0:row0 + nrows]), (row0, nrows)
        assert np.all(_fetch(ctx, 17, 0, n) == -7.0)                        # no rows: nothing is written
        am.assert_untouched(store, snap)


def test_row_fetch_in_three_blocks(hic):
    """n = 4099: a 64 MiB block is 2046 rows, so the strided copy loop takes three rounds (2046 + 2046 + 7)."""
    n = 4099
    assert ((64 << 20) // (8 * n)) == 2046 and 2 * 2046 < n < 3 * 2046
    M = np.random.default_rng(32).random((n, n))
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, M, "odd")
        assert _same_bits(ctx.contacts_host(), M)
        assert _same_bits(_fetch(ctx, 2040, 2052, n), M[2040:4092])         # a piece of two rounds that starts mid-block
        am.assert_untouched(store, snap)


# --------------------------------------------------------------------------------- compact
def _keep_lists(n):
    dropped = np.random.default_rng(n).choice(np.arange(1, n - 1), size=n // 5, replace=False)      # scattered, interior
    return {"first dropped": np.arange(1, n), "last dropped": np.arange(n - 1),
            "interior dropped": np.setdiff1d(np.arange(n), dropped)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [50, 300])
def test_compact(hic, orc, layout, n):
    rng = np.random.default_rng(3 + n)
    m = rng.random((n, n)); m = m + m.T
    for what, keep in _keep_lists(n).items():
        keep = keep.astype(np.int32)
        sub = np.ascontiguousarray(m[np.ix_(keep, keep)])
        with hic.Context(0) as ctx:
            store, snap = am.adopt(ctx, m, layout)
            ctx.compact(keep)
            assert _same_bits(ctx.contacts_host(), sub), what
            ptr, n_now, ld_now = ctx.contacts_device()
            assert (n_now, ld_now) == (len(keep), len(keep)), what              # the copy is the context's own, dense
            assert not (store.data_ptr() <= ptr < store.data_ptr() + 8 * store.numel())
            np_sum, seq = ctx.row_sums()
            am.assert_untouched(store, snap)
        assert np.array_equal(np_sum, orc.np_row_sums(sub)), what
        assert np.array_equal(seq, orc.seq_row_sums(sub)), what


# --------------------------------------------------------------------------------- UPGMA
@functools.lru_cache(maxsize=None)
def _upgma_case(n, seed):
    """The matrix of test_upgma_random_bit_exact and the oracle's raw merges, leaf order and linkage."""
    import hic_oracle as orc
    rng = np.random.default_rng(seed)
    c = rng.random((n, n)) + 0.01
    c = c + c.T
    dist = orc.to_distance(c)
    zraw = orc.nn_chain_raw(dist)
    leaves, z = orc.average_cluster_leaves(dist)
    return c, zraw, leaves, z


def _check_upgma(ctx, layout, n, seed):
    c, zraw_o, leaves_o, z_o = _upgma_case(n, seed)
    store, snap = am.adopt(ctx, c, layout, "finite")
    leaves, z = ctx.upgma()
    zraw = ctx.raw_merges()
    assert np.array_equal(zraw, zraw_o)                  # merge order, pairs, heights, sizes: bit for bit
    assert np.array_equal(z, z_o)
    assert np.array_equal(leaves, leaves_o)
    return store, snap, c, leaves


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,seed", [(2, 0), (65, 4), (333, 5), (1025, 6)])
def test_upgma(hic, layout, n, seed, monkeypatch):
    monkeypatch.delenv("HICMI_PRESORT_FROM", raising=False)
    with hic.Context(0) as ctx:
        store, snap, _c, _leaves = _check_upgma(ctx, layout, n, seed)
        am.assert_untouched(store, snap)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_upgma_with_the_presort_beside_the_chain(hic, layout, monkeypatch):
    """HICMI_PRESORT_FROM below n: every row of the adopted matrix is also sorted on the second stream while the chain
    runs.  The merges are the oracle's, and so is the rank matrix hicmi_rank_matrix makes of the pre-sorted rows (random
    contacts: next to no equal similarities, the rows are only re-addressed by the leaf order)."""
    n, seed = 1025, 6
    for var in ("HICMI_NO_PRESORT", "HICMI_SORT_RADIX", "HICMI_SORT_LDS", "HICMI_PRESORT_TIES"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("HICMI_PRESORT_FROM", "64")
    with hic.Context(0) as ctx:
        store, snap, c, leaves = _check_upgma(ctx, layout, n, seed)
        ctx.rank_matrix(leaves)
        state, n_tied = ctx.presort_state()
        assert state == 1 and n_tied <= 3 + n // 400
        _check_rank(ctx, "upgma %d %d" % (n, seed), c, leaves, "pre-sort, " + layout)
        am.assert_untouched(store, snap)


# --------------------------------------------------------------------------------- rank matrix, similarity row
RANK_SIZES = [100, 1000, 2500]
RANK_KINDS = ["random", "quantised"]
_rank_oracle_cache = {}


def _rank_contacts(n, kind):
    """random: the matrix of test_rank_matrix_bit_exact; quantised: that of test_rank_matrix_tie_rule (heavy ties)."""
    rng = np.random.default_rng(1000 + n if kind == "random" else 2000 + n)
    if kind == "random":
        c = rng.random((n, n)) + 0.01
        c = c + c.T
    else:
        c = rng.integers(0, 5, size=(n, n)).astype(np.float64)
        c = np.triu(c, 1) + np.triu(c, 1).T + np.eye(n) * 3
    return c, rng.permutation(n).astype(np.int32)


def _rank_oracle(key, c, order):
    """(similarity matrix in ``order``, argsort rows) of the oracle for the contacts ``c`` that ``key`` names, computed
    once per matrix and order (as _oracle_rank of test_gpu_parity.py)."""
    import hic_oracle as orc
    order = np.ascontiguousarray(order, dtype=np.int32)
    key = (key, order.tobytes())
    if key not in _rank_oracle_cache:
        n = len(c)
        bins = [orc.Bin(i, "s", 0, 0, 0.0, 0.0) for i in range(n)]
        mat, bins = orc.remove_zero_rows(c.copy(), bins)
        assert len(mat) == n
        dist = orc.to_distance(mat)
        dist = dist[:, order][order]
        sim = orc.to_similarity(dist, [bins[i] for i in order])
        _rank_oracle_cache[key] = (sim, np.ascontiguousarray(orc.rank_order(sim)).astype(np.uint16))
    return _rank_oracle_cache[key]


def _rank_probe_rows(n):
    rng = np.random.default_rng(n)
    return np.unique(np.concatenate([np.arange(min(n, 40)), rng.integers(0, n, 40), [n - 1]]))


def _probe3(rows):
    return [int(rows[0]), int(rows[-1]), int(rows[len(rows) // 2])]


def _check_rank(ctx, key, c, order, what):
    """The checks of test_rank_matrix_bit_exact and test_rank_matrix_tie_rule on the context's rank matrix."""
    n = len(c)
    sim, R_o = _rank_oracle(key, c, order)
    R = ctx.rank_rows()
    inv = ctx.rank_rows(inverse=True)
    rows = _rank_probe_rows(n)
    assert np.array_equal(R, R_o), what
    for r in _probe3(rows):
        assert np.array_equal(ctx.similarity_row(r), sim[r]), (what, r)
    ar = np.arange(n)
    for r in rows:
        assert np.array_equal(inv[r][R[r]], ar), (what, r)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", RANK_SIZES)
@pytest.mark.parametrize("kind", RANK_KINDS)
def test_rank_matrix_per_call_sorters(hic, layout, kind, n, monkeypatch):
    """The default register-blocked bitonic sorter and HICMI_SORT_RADIX=1: both switches are read in every
    hicmi_rank_matrix call (tests/test_adopted_cpu.py checks that in the source), so one process runs both."""
    monkeypatch.delenv("HICMI_SORT_LDS", raising=False)
    monkeypatch.delenv("HICMI_SORT_RADIX", raising=False)
    c, order = _rank_contacts(n, kind)
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, c, layout, "finite")
        ctx.rank_matrix(order)
        assert ctx.presort_state() == (0, 0)
        _check_rank(ctx, (kind, n), c, order, "default")
        monkeypatch.setenv("HICMI_SORT_RADIX", "1")
        ctx.rank_matrix(order)
        _check_rank(ctx, (kind, n), c, order, "radix")
        am.assert_untouched(store, snap)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", RANK_SIZES)
def test_rank_matrix_after_the_presort(hic, layout, n, monkeypatch):
    """upgma() with HICMI_PRESORT_FROM lowered sorts the adopted rows beside the chain; on quantised contacts every row
    holds equal similarities, so hicmi_rank_matrix finishes all of them with k_rank_rows_tied."""
    monkeypatch.delenv("HICMI_SORT_LDS", raising=False)
    monkeypatch.delenv("HICMI_SORT_RADIX", raising=False)
    monkeypatch.delenv("HICMI_NO_PRESORT", raising=False)
    monkeypatch.delenv("HICMI_PRESORT_TIES", raising=False)
    monkeypatch.setenv("HICMI_PRESORT_FROM", "64")
    c, _order = _rank_contacts(n, "quantised")
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, c, layout, "finite")
        leaves, _z = ctx.upgma(want_linkage=False)
        ctx.rank_matrix(leaves)
        assert ctx.presort_state() == (1, n)                      # the pre-sort was used, every row went to the tied kernel
        _check_rank(ctx, ("quantised", n), c, leaves, "pre-sort")
        am.assert_untouched(store, snap)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


CHILD = ("import sys; sys.path[:0] = [%r, %r, %r]; import test_gpu_adopted_ld as t; t.child_main(int(sys.argv[1]))"
         % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")))


def child_main(n):
    """HICMI_SORT_LDS is read once per process: this runs in a fresh child with the switch set.  One JSON line per kind and
    layout with the digests of the argsort rows, the rank rows and three similarity rows."""
    import torch
    from hic_genome_assembler_amd import _lib
    assert os.environ.get("HICMI_SORT_LDS")
    rows = _rank_probe_rows(n)
    for kind in RANK_KINDS:
        c, order = _rank_contacts(n, kind)
        for layout in LAYOUTS:
            with _lib.Context(0) as ctx:
                store, snap = am.adopt(ctx, c, layout, "finite")
                ctx.rank_matrix(order)
                R, inv = ctx.rank_rows(), ctx.rank_rows(inverse=True)
                sims = [ctx.similarity_row(r) for r in _probe3(rows)]
                torch.cuda.synchronize()
                untouched = bool(torch.equal(store.view(torch.int64), snap))
            print(json.dumps({"kind": kind, "layout": layout, "R": _digest(R), "inv": _digest(inv),
                              "sims": [_digest(s) for s in sims], "untouched": untouched}))


@pytest.mark.parametrize("n", RANK_SIZES)
def test_rank_matrix_lds_sorter_in_a_fresh_process(n):
    env = {k: v for k, v in os.environ.items() if k not in ("HICMI_SORT_RADIX", "HICMI_NO_PRESORT", "HICMI_PRESORT_FROM")}
    env["HICMI_SORT_LDS"] = "1"
    res = subprocess.run([sys.executable, "-c", CHILD, str(n)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    assert [(g["kind"], g["layout"]) for g in got] == [(k, lay) for k in RANK_KINDS for lay in LAYOUTS]
    rows = _rank_probe_rows(n)
    for g in got:
        c, order = _rank_contacts(n, g["kind"])
        sim, R_o = _rank_oracle((g["kind"], n), c, order)
        inv_o = np.empty_like(R_o)
        np.put_along_axis(inv_o, R_o.astype(np.int64), np.arange(n, dtype=np.uint16)[None, :], axis=1)
        what = (g["kind"], g["layout"])
        assert g["R"] == _digest(R_o), what
        assert g["inv"] == _digest(inv_o), what
        assert g["sims"] == [_digest(sim[r]) for r in _probe3(rows)], what
        assert g["untouched"], what


# --------------------------------------------------------------------------------- Part 2 objective
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_used", [2, 9, 130])
def test_p2_literal_scores(hic, orc, layout, n_used):
    """test_p2_literal_scores_bit_exact on a permuted sub-list of an adopted 400-bin map."""
    n = 400
    rng = np.random.default_rng(n_used)
    m = rng.random((n, n)) * 7.0; m = m + m.T
    sel = rng.permutation(n)[:n_used].astype(np.int32)
    perms = np.stack([rng.permutation(n_used) for _ in range(9)]).astype(np.int32)
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, m, layout)
        ctx.p2_select(sel)
        total = ctx.p2_total()
        exact = ctx.p2_score_exact(perms, total)
        fast = ctx.p2_score(perms, total)
        am.assert_untouched(store, snap)
    L = orc.lib()
    assert total == L.hio_total_upper(orc._dp(m), n, orc._ip(sel), n_used)
    assert exact.tolist() == orc.cost_literal_rows(m, sel[perms], total).tolist()
    print("p2 %s n_used %d: largest |fast - exact| / |exact| = %.3e (bound 1e-11)"
          % (layout, n_used, float(np.max(np.abs(fast - exact) / np.abs(exact)))))
    assert np.allclose(fast, exact, rtol=1e-11, atol=0)


# --------------------------------------------------------------------------------- plots
def _plot_maps():
    c = gc.load_case("n300_edges")[4]
    rng = np.random.default_rng(257)
    r = rng.random((257, 257)) * 20.0 + 0.01
    return {"n300_edges": c, "random257": np.ascontiguousarray(r + r.T)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["n300_edges", "random257"])
def test_plot_percentiles_and_downsample(hic, layout, name):
    """n300_edges has empty bins: the row sums and hicmi_compact read the adopted source and the plots the compacted
    copy; the 257-bin map stays adopted.  References as in test_plot_percentiles_and_downsample of test_gpu_parity.py."""
    c = _plot_maps()[name]
    rng = np.random.default_rng(21)
    worst = 0.0
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, c, layout)
        np_sum, seq_sum = ctx.row_sums()
        assert np.array_equal(np_sum, c.sum(axis=1))
        if name == "n300_edges":
            assert np.any(np_sum == 0)
            keep = np.flatnonzero(np_sum != 0)
            ctx.compact(keep)
            c = np.ascontiguousarray(c[np.ix_(keep, keep)])
            np_sum, seq_sum = ctx.row_sums()
        else:
            assert ctx.contacts_device()[2] > len(c)                          # still the caller's storage
        n = len(c)
        dist = (1.0 - c / np_sum[:, None]) + 1.0
        sim = seq_sum[:, None] * (1.0 - (dist - 1.0))
        perm = rng.permutation(n).astype(np.int32)
        sub = np.sort(rng.choice(n, size=n // 3, replace=False)).astype(np.int32)[::-1].copy()
        q = [1, 98, 0, 100, 50, 33.3]
        for kind, mat in ((0, c), (1, dist), (2, sim)):
            for order in (None, perm, sub):
                view = mat if order is None else mat[np.ix_(order, order)]
                got = ctx.plot_percentiles(kind, order, q)
                want = np.percentile(view, q)
                assert np.array_equal(got, want), (name, kind, got, want)
                m = len(view)
                for px in (m, 7, 64):
                    img = ctx.plot_downsample(kind, order, px)
                    edges = (np.arange(px + 1, dtype=np.int64) * m) // px
                    rows = np.add.reduceat(view, edges[:-1], axis=0)
                    blocks = np.add.reduceat(rows, edges[:-1], axis=1)
                    cnt = np.diff(edges)
                    ref = blocks / (cnt[:, None] * cnt[None, :])
                    assert np.allclose(img, ref, rtol=1e-12, atol=0), (name, kind, px)
                    nz = ref != 0
                    worst = max(worst, float(np.max(np.abs(img[nz] - ref[nz]) / np.abs(ref[nz]))))
        am.assert_untouched(store, snap)
    print("plot %s %s: largest relative deviation of a block mean %.3e (bound 1e-12)" % (name, layout, worst))


# --------------------------------------------------------------------------------- HMM observations
HMM_N = 600
HMM_WINDOWS = [(0, HMM_N), (0, 40), (HMM_N // 3, HMM_N // 3 + 63), (HMM_N - 30, HMM_N)]


@pytest.fixture(scope="module")
def hmm_case(hic):
    """The 600-bin map of test_observations_equal_the_log_similarity, its leaf order, the reference log-similarity and
    the observations a context that owns a dense copy loads."""
    from hic_genome_assembler_amd import synth
    C = synth.dense_contacts(synth.make_layout(HMM_N, seed=2), seed=2)
    owned = {}
    with hic.Context(0) as ctx:
        ctx.set_contacts(C)
        ctx.row_sums()
        leaves, _z = ctx.upgma(want_linkage=False)
        leaves = np.asarray(leaves)
        for c, p in HMM_WINDOWS:
            ctx.hmm_load_obs(leaves, c, p)
            owned[(c, p)] = ctx.hmm_get_obs()
    return C, leaves, href.log_similarity(C, leaves), owned


@pytest.mark.parametrize("layout", LAYOUTS)
def test_hmm_observations(hic, hmm_case, layout):
    C, leaves, A, owned = hmm_case
    worst = 0
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, C, layout)
        ctx.row_sums()
        for c, p in HMM_WINDOWS:
            want = A[c:, c:p]
            ctx.hmm_load_obs(leaves, c, p)
            X = ctx.hmm_get_obs()
            ctx.hmm_load_obs_slot(3, leaves, c, p)
            ctx.hmm_use_obs(3)
            X3 = ctx.hmm_get_obs()
            ctx.hmm_use_obs(0)
            for got in (X, X3):
                assert got.shape == want.shape
                worst = max(worst, int(_ulps(got, want).max()))
                assert int(_ulps(got, want).max()) <= 2, (c, p)
                assert _same_bits(got, owned[(c, p)]), (c, p)
        am.assert_untouched(store, snap)
    print("hmm observations %s: largest distance from the reference %d ulps (bound 2)" % (layout, worst))


# --------------------------------------------------------------------------------- Louvain graph
@pytest.fixture(scope="module")
def louvain_case(hic):
    """test_graph_build_n400_tail: the last 13 % of n400_default in its dendrogram order, the reference graph and what a
    context that owns a dense copy builds."""
    from hic_genome_assembler_amd import modularity as mod
    C = gc.load_case("n400_default")[4]
    with hic.Context(0) as ctx:
        ctx.set_contacts(C)
        ctx.row_sums()
        leaves, _z = ctx.upgma(want_linkage=False)
        leaves = np.asarray(leaves)
        start = int(len(C) * 0.87)
        ctx.louvain_graph(leaves[start:])
        owned = ctx.louvain_get_graph()
    return C, leaves[start:], mod.graph_weights(href.log_similarity(C, leaves)[start:, start:]), owned


@pytest.mark.parametrize("layout", LAYOUTS)
def test_louvain_graph(hic, louvain_case, layout):
    from hic_genome_assembler_amd import modularity as mod
    C, rows, want, owned = louvain_case
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, C, layout)
        ctx.row_sums()
        ctx.louvain_graph(rows)
        A, gdeg, total = ctx.louvain_get_graph()
        am.assert_untouched(store, snap)
    print("louvain graph %s: largest distance from the reference %d ulps (bound 2)" % (layout, int(_ulps(A, want).max())))
    assert int(_ulps(A, want).max()) <= 2
    assert np.array_equal(A, A.T)
    st = mod._Status(A.copy())
    assert total == st.total_weight and np.array_equal(gdeg, st.gdegrees)
    assert _same_bits(A, owned[0]) and _same_bits(gdeg, owned[1]) and total == owned[2]


# --------------------------------------------------------------------------------- worker contexts, Part 2 reports
def _same_result(a, b, path="result"):
    """Nested dicts / lists / arrays / numbers equal bit for bit."""
    if isinstance(a, dict):
        assert isinstance(b, dict) and sorted(a) == sorted(b), path
        for k in a:
            _same_result(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same_result(x, y, "%s[%d]" % (path, i))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and _same_bits(a, b), path
    elif isinstance(a, float):
        assert isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes(), path
    else:
        assert a == b, path


def _reports(ctx, case):
    """The four support reports of Part 2 on ``ctx``: placement, breaks and inversions go through one
    hicmi_p2_*_multi call each with one worker context per chromosome, the junctions through hicmi_junction_sums."""
    from hic_genome_assembler_amd import orderGenome as p2
    binList, chromList, groups, orders = case["binList"], case["chromList"], case["groups"], case["orders"]
    out = {}
    for name, fn in (("support", p2.placementSupport), ("breaks", p2.breakSupport), ("inversions", p2.inversionSupport),
                     ("junctions", p2.junctionSupport)):
        ordered = _quiet(p2.scaffoldsFromOrderFile, chromList, orders)
        out[name] = _quiet(fn, p2.GenomeMatrix(ctx), ordered, binList, chromList)
    return out, len(ordered)


@pytest.fixture(scope="module")
def n600_groups(hic, tmp_path_factory):
    """n600 restricted to the bins of Part 1's groups, as -part2 loads it, and the reports of a context that owns it."""
    from hic_genome_assembler_amd import orderGenome as p2
    from hic_genome_assembler_amd.hostio import initiateLoci, read_contact_matrix
    name = "n600"
    paths = _quiet(gc.write_case_files, name, str(tmp_path_factory.mktemp("n600_groups")))
    groups = os.path.join(gc.GOLDEN_DIR, name, "chromosomeGroups.txt")
    orders = os.path.join(gc.GOLDEN_DIR, name, "chromosomeOrders.txt")
    binList = initiateLoci(paths["hicProBedFile"], paths["hicProBiasFile"], binID_dict=p2.readGroupingsToValidBins(groups))
    host = read_contact_matrix(paths["hicProMatrixFile"], binList)
    case = dict(binList=binList, chromList=_quiet(p2.readChromsFromFile, groups), groups=groups, orders=orders, host=host)
    with hic.Context(0) as ctx:
        ctx.set_contacts(host)
        case["owned"], case["chromosomes"] = _reports(ctx, case)
    assert case["chromosomes"] > 1                                         # so the reports do run on worker contexts
    return case


@pytest.mark.parametrize("layout", LAYOUTS)
def test_workers_reports_equal_an_owned_copy(hic, n600_groups, layout):
    case = n600_groups
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, case["host"], layout, "finite")
        parent = ctx.contacts_device()
        assert parent[2] > parent[1]
        workers = ctx.workers(3)
        assert len(workers) == 3
        for w in workers:
            assert w.contacts_device() == parent                          # same address, same n, same ld: no copy
        got, _n = _reports(ctx, case)
        for w in ctx.workers(case["chromosomes"] - 1):
            assert w.contacts_device() == parent
        am.assert_untouched(store, snap)
    for name in ("support", "breaks", "inversions", "junctions"):
        _same_result(got[name], case["owned"][name], name)


# --------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("layout", ["odd", "block"])
@pytest.mark.parametrize("name", ["n600", "n300_edges"])
def test_resident_pipeline_on_an_adopted_matrix(hic, layout, name, tmp_path, monkeypatch):
    """test_resident_path_with_background_file_writer with the map adopted instead of uploaded.  n600 has no empty bins:
    Part 1, the pre-sort beside the chain (HICMI_PRESORT_FROM lowered) and every Part 2 job on the worker contexts read
    the caller's storage with ld > n; n300_edges compacts from it first."""
    from hic_genome_assembler_amd import orderGenome as p2, scaffoldToChromosomes as p1
    from hic_genome_assembler_amd.hostio import initiateLoci, read_contact_matrix
    monkeypatch.setenv("HICMI_PRESORT_FROM", "64")
    spec = gc.load_case(name)[0]
    paths = gc.write_case_files(name, str(tmp_path))
    f = lambda k: os.path.join(str(tmp_path), k)  # noqa: E731
    bins = initiateLoci(paths["hicProBedFile"], paths["hicProBiasFile"])
    host = read_contact_matrix(paths["hicProMatrixFile"], bins)
    ctx = hic.Context(0)
    try:
        store, snap = am.adopt(ctx, host, layout, "finite")
        dm = p1.DeviceMatrix(ctx)
        p1.runResident(dm, bins, paths["hicProScaffSizeFile"], f("dendrogramOrder.txt"), f("binGroups.txt"),
                       f("assessment.txt"), f("chromosomeGroups.txt"), spec["min_size"], 0.0, spec["psig"], overlap_files=True)
        assert dm.chromosome_groups is not None
        adopted_still = ctx.contacts_device()[2] > ctx.n
        assert adopted_still == (name == "n600")
        if name == "n600":
            assert ctx.presort_state()[0] == 1
        p2.runResident(p2.GenomeMatrix(dm.ctx), dm.kept_bins, f("chromosomeGroups.txt"), f("chromosomeOrders.txt"),
                       f("plotOrder.txt"), spec["n_scaffolds"], spec["scan_scaffolds"], 100000,
                       chromosomeList=dm.chromosome_groups, on_native_phase=dm.release_files)
        dm.finish_files()
        am.assert_untouched(store, snap)
    finally:
        ctx.close()
    for fn in gc.OUTPUT_FILES:
        with open(f(fn)) as fh:
            assert fh.read() == gc.golden_text(name, fn), fn


# --------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_matrix_in_place(hic):
    """ld < n and a NULL pointer are HICMI_EINVAL; the matrix adopted before stays set and usable."""
    import torch
    n = 129
    m, _rows, np_ref, seq_ref = _row_sum_case(n)
    lib = hic.load()
    with hic.Context(0) as ctx:
        store, snap = am.adopt(ctx, m, "odd")
        before = ctx.contacts_device()
        other = torch.zeros(n * n, dtype=torch.float64, device="cuda:0")
        assert lib.hicmi_set_contacts_device(ctx._h, ctypes.c_void_p(other.data_ptr()), n, n - 1) == EINVAL     # ld < n
        assert lib.hicmi_set_contacts_device(ctx._h, ctypes.c_void_p(None), n, n) == EINVAL                     # NULL
        assert ctx.contacts_device() == before
        np_sum, seq = ctx.row_sums()
        am.assert_untouched(store, snap)
    assert np.array_equal(np_sum, np_ref) and np.array_equal(seq, seq_ref)
