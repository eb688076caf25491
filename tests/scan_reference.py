"""Crafted rank matrices and exact references for Part 1's scan loops and the device hypergeometric test.

Nothing here needs a GPU.  tests/test_scan_cpu.py shows, from the oracle alone, that every case reaches the branch it
is named for and that no decision of the grid hinges on rounding; tests/test_gpu_scan.py runs the same cases on the
device.

Planting a rank matrix: the sort kernels read the contact matrix row by row and the similarity transform scales a row by
its own sums only, so with the identity leaf order and C[i, R[i, k]] = n - k the device's argsort rows are R itself
(contacts_for_ranks; the GPU tests assert that before anything else).

The exact tail: P[X >= x], X ~ Hypergeom(M, n, N), as a ratio of Python integers - one math.comb product for the first
term of the support, the exact integer recurrence w_{k+1} = w_k (n-k)(N-k) // ((k+1)(M-n-N+k+1)) for the others,
suffix sums, and math.comb(M, N) as the denominator.  A comparison with psig is a comparison of integers (psig is the
exact value of the double), so neither the decisions nor the margins below carry any rounding.
"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

PSIGS = (.05, .01, 1e-6)
MARGIN = Fraction(1, 10 ** 6)           # no exact tail of the grid lies this close (relative) to its psig


# ------------------------------------------------------------------------------------------------ planting
def contacts_for_ranks(R):
    """The contact matrix whose rank matrix (identity leaf order, no upgma() before rank_matrix()) is R: row i of R is
    a permutation of 0..n-1 and C[i, R[i, k]] = n - k - positive, distinct within a row, integers."""
    R = np.asarray(R, dtype=np.int64)
    n = R.shape[0]
    assert R.shape == (n, n) and np.array_equal(np.sort(R, axis=1), np.broadcast_to(np.arange(n), (n, n)))
    C = np.empty((n, n), dtype=np.float64)
    C[np.arange(n)[:, None], R] = (n - np.arange(n, dtype=np.float64))[None, :]
    return C


# ------------------------------------------------------------------------------------------------ exact tail
def _suffix_sums(M, n, N):
    """(lo, S) with S[k - lo] = sum_{j >= k} C(n, j) C(M - n, N - j) for k in lo..hi; None for invalid arguments
    (SciPy's hypergeom._argcheck: the tail is NaN)."""
    if not (M > 0 and 0 <= n <= M and 0 <= N <= M):
        return None
    lo, hi = max(0, N - (M - n)), min(n, N)
    w = math.comb(n, lo) * math.comb(M - n, N - lo)
    ws = [w]
    for k in range(lo, hi):
        w = w * (n - k) * (N - k) // ((k + 1) * (M - n - N + k + 1))         # exact: w_{k+1} is an integer
        ws.append(w)
    S = ws
    for k in range(len(S) - 2, -1, -1):
        S[k] += S[k + 1]
    return lo, S


Tail = namedtuple("Tail", "lo hi S T")      # S[x - lo] / T = P[X >= x] for lo <= x <= hi


@functools.lru_cache(maxsize=64)
def exact_table(M, n, N):
    """The whole table of one (M, n, N): None when the arguments are invalid."""
    got = _suffix_sums(M, n, N)
    if got is None:
        return None
    lo, S = got
    return Tail(lo, lo + len(S) - 1, S, math.comb(M, N))


def exact_sf(x, M, n, N):
    """hyper_geom(x, M, n, N) of the reference, exactly: a Fraction, or None where SciPy gives NaN."""
    t = exact_table(M, n, N)
    if t is None:
        return None
    if x <= t.lo:
        return Fraction(1)
    if x > t.hi:
        return Fraction(0)
    return Fraction(t.S[x - t.lo], t.T)


def _cmp_parts(x, t, psig):
    """(a, b) with sign(a - b) = sign(P[X >= x] - psig), integers."""
    p = Fraction(psig)                                   # the exact value of the double
    if x <= t.lo:
        s, T = 1, 1
    elif x > t.hi:
        s, T = 0, 1
    else:
        s, T = t.S[x - t.lo], t.T
    return s * p.denominator, p.numerator * T


def exact_below(x, M, n, N, psig):
    """hyper_geom(x, M, n, N) < psig, exactly; None for NaN."""
    t = exact_table(M, n, N)
    if t is None:
        return None
    a, b = _cmp_parts(x, t, psig)
    return a < b


def exact_gap(x, M, n, N, psig):
    """|P[X >= x] - psig| / psig as a Fraction (None for NaN)."""
    t = exact_table(M, n, N)
    if t is None:
        return None
    a, b = _cmp_parts(x, t, psig)
    return Fraction(abs(a - b), b)


def _x_star(t, psig):
    """Smallest x with P[X >= x] < psig (the tail falls with x; hi + 1 gives 0)."""
    a, b = t.lo, t.hi + 1                                # P(a) = 1 >= psig, P(b) = 0 < psig
    while b - a > 1:
        mid = (a + b) // 2
        u, v = _cmp_parts(mid, t, psig)
        if u < v:
            b = mid
        else:
            a = mid
    return b


GridPoint = namedtuple("GridPoint", "M L lo hi x_star gap")     # x_star, gap: one entry per psig of PSIGS


@functools.lru_cache(maxsize=None)
def grid_point(M, L):
    """Thresholds of the row test hyper_geom(x, M, L, L) at every psig: x_star[k] is the smallest significant count,
    gap[k] the smaller relative distance to psig of the tails at x_star and x_star - 1 (the tail is monotone in x, so
    every other x is farther away).  None when M < L (NaN)."""
    got = _suffix_sums(M, L, L)
    if got is None:
        return None
    lo, S = got
    t = Tail(lo, lo + len(S) - 1, S, math.comb(M, L))
    stars, gaps = [], []
    for psig in PSIGS:
        xs = _x_star(t, psig)
        g = []
        for x in (xs - 1, xs):
            a, b = _cmp_parts(x, t, psig)
            g.append(Fraction(abs(a - b), b))
        stars.append(xs)
        gaps.append(float(min(g)))
    return GridPoint(M, L, t.lo, t.hi, tuple(stars), tuple(gaps))


def grid_flag(x, M, L, psig, mode):
    """The flag of a row that counts x: mode 0 (first pass) 0 where the tail is >= psig and 1 otherwise, NaN included;
    mode 1 (filter) 1 where the tail is < psig and 0 otherwise, NaN included."""
    gp = grid_point(M, L)
    if gp is None:
        return 1 if mode == 0 else 0
    return 1 if x >= gp.x_star[PSIGS.index(psig)] else 0


# ------------------------------------------------------------------------------------------------ the grid
GRID_N = 4096
GRID_M = (4096, 5000, 16000, 65535)
GRID_L_ALL = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200, 511, 512, 1000, 2047, 2048, 3000, 4095)
GRID_L_DEVICE = tuple(L for L in GRID_L_ALL if L <= GRID_N // 2)      # what one filter_scan(0, L, L + 1, ..) can plant
# beside the measured grid: 2L > M (the support starts above 0) and M < L (NaN) - part of the margin proof as well
GRID_EXTRA = ((3000, 2047), (3000, 2048), (2100, 2048), (600, 511), (600, 512), (100, 63), (100, 64), (100, 65),
              (64, 64), (65, 64), (100, 200), (63, 64), (2047, 2048), (1, 2))


def grid_points_device():
    return [(M, L) for M in GRID_M for L in GRID_L_DEVICE] + list(GRID_EXTRA)


def grid_points_cpu():
    return [(M, L) for M in GRID_M for L in GRID_L_ALL] + list(GRID_EXTRA)


@functools.lru_cache(maxsize=1)
def grid_ranks():
    """n = 4096; row i ranks the columns 0..i-1 first, ascending, then n-1, n-2, .., i.  With start = 0 and cut = L the
    filter's row test counts #{v in R[i, :L] : 0 <= v <= L} = min(i, L) for L < n/2 - one scan of the rows 0..L plants
    every x of 0..L.  (At L = n/2 row 0 counts 1: its first n/2 ranks cannot avoid n/2 + 1 columns.)"""
    n = GRID_N
    R = np.empty((n, n), dtype=np.int64)
    for i in range(n):
        R[i, :i] = np.arange(i)
        R[i, i:] = np.arange(n - 1, i - 1, -1)
    return R


def mode1_counts(R, start, c, n_rows):
    """S2C:626-631 as the oracle counts: x of the rows start .. start + n_rows - 1 for the candidate c."""
    local = c - start
    sub = R[start:start + n_rows, :local]
    return np.count_nonzero((sub >= start) & (sub <= c), axis=1).astype(np.int64)


def mode0_counts(R, start):
    """S2C:455-459: entry t counts #{v in R[start + t, :t] : start <= v <= start + t}; entry 0 is 0."""
    n = R.shape[0]
    out = np.zeros(n - start, dtype=np.int64)
    for t in range(1, n - start):
        pr = R[start + t, :t]
        out[t] = np.count_nonzero((pr >= start) & (pr <= start + t))
    return out


MODE0_N = 769                           # entries t = 0..768: L = t
# The matrix is built for the first M, the map's own size (what the loop passes at start 0; a row's count is then at
# least the support's lower end + 1, so nearly every threshold can be planted).  500 < t gives NaN rows and 2t > M from
# 251 on; at 4096 the same counts lie far above the thresholds.
MODE0_M = (769, 500, 4096)


@functools.lru_cache(maxsize=None)
def mode0_ranks(psig):
    """The first pass's row test near its threshold in every row: row t holds x*(M0, t, psig) - 1 + (t mod 3) of the
    columns 0..t among its first t ranks (clipped to what a row can hold), so cut_scan(0, M0, psig) sees counts just
    below, at and just above the smallest significant one, with L = t for every t."""
    n, M0 = MODE0_N, MODE0_M[0]
    assert M0 == n
    k = PSIGS.index(psig)
    R = np.empty((n, n), dtype=np.int64)
    R[0] = np.arange(n)
    for t in range(1, n):
        x = grid_point(M0, t).x_star[k] - 1 + (t % 3)
        x = max(x, 2 * t + 1 - n, 0)                     # the first t ranks hold at least t - (n - t - 1) of 0..t
        x = min(x, t)
        inside = list(range(x))                          # x of the columns 0..t, then t - x columns beyond t
        outside = list(range(t + 1, t + 1 + (t - x)))
        head = inside + outside
        rest = [v for v in range(n - 1, -1, -1) if v >= x and not (t < v <= t + (t - x))]
        R[t] = head + rest
    return R


# ------------------------------------------------------------------------------------------------ loop cases
def block_ranks(n, bounds, reverse_rows=(), far_rows=()):
    """Blocks [b, e) between consecutive bounds: row i of a block ranks i, i-1, .., b, then i+1, .., e-1, then the columns
    right of the block from n-1 down and those left of it from b-1 down.  From the block's own start every row counts
    the maximum.  Rows that break the pattern: ``reverse_rows`` rank in the opposite order (their own block last),
    ``far_rows`` rank n-1, n-2, .., 0."""
    R = np.empty((n, n), dtype=np.int64)
    edges = [0] + list(bounds) + [n]
    for b, e in zip(edges[:-1], edges[1:]):
        assert b < e
        for i in range(b, e):
            R[i] = list(range(i, b - 1, -1)) + list(range(i + 1, e)) + list(range(n - 1, e - 1, -1)) + list(range(b - 1, -1, -1))
    for i in reverse_rows:
        R[i] = R[i][::-1].copy()
    for i in far_rows:
        R[i] = np.arange(n - 1, -1, -1)
    return R


def shared_block_ranks(n, bounds, far_rows=()):
    """Every row of a block [b, e) ranks b, b+1, .., e-1 first (the same for all of them), then n-1 down to e, then b-1
    down to 0: a candidate inside a block flags every row of the block."""
    R = np.empty((n, n), dtype=np.int64)
    edges = [0] + list(bounds) + [n]
    for b, e in zip(edges[:-1], edges[1:]):
        R[b:e] = np.array(list(range(b, e)) + list(range(n - 1, e - 1, -1)) + list(range(b - 1, -1, -1)))
    for i in far_rows:
        R[i] = np.arange(n - 1, -1, -1)
    return R


def shrinking_ranks(n, s, M_sig, M_not):
    """One cut at s, then rows built around the second start: row s + t holds the smallest count that is significant at
    M_sig (psig .05).  At the smaller M_not more than a tenth of those counts must no longer be significant (asserted
    here, on the exact tails), so the >= 90 % rule that fires at M_sig cannot fire again at M_not."""
    R = block_ranks(n, [s])
    lost = 0
    for t in range(1, n - s):
        i = s + t
        gp = grid_point(M_sig, t)
        x = t if gp is None else min(gp.x_star[0], t)
        x = max(x, 2 * t + 1 - (n - s), 0)
        lost += grid_flag(x, M_sig, t, .05, 0) == 1 and grid_flag(x, M_not, t, .05, 0) == 0
        inside = list(range(i, i - x, -1))                       # x of the columns s..i
        outside = [v for v in range(i + 1, n)][: t - x]
        outside += list(range(s - 1, -1, -1))[: t - x - len(outside)]
        head = inside + outside
        assert len(head) == t, (n, s, t, x)
        seen = set(head)
        R[i] = head + [v for v in range(n - 1, -1, -1) if v not in seen]
    assert 10 * lost > n - s, (n, s, M_sig, M_not, lost)
    return R


def stop_index(n, min_frac):
    return int(n - (n * min_frac))                               # S2C:519, as the reference rounds it


@functools.lru_cache(maxsize=None)
def ranks(name):
    return MAPS[name]()


MAPS = {
    "n2": lambda: block_ranks(2, []),
    "n3": lambda: block_ranks(3, [1]),
    "n11": lambda: block_ranks(11, [6]),
    # bounds with every residue mod 8 (the 16-byte count loop starts at lo = the previous cut): 0 9 18 27 36 45 54 63
    "n77-residues": lambda: block_ranks(77, [9, 18, 27, 36, 45, 54, 63], reverse_rows=(30,), far_rows=(50,)),
    # bounds 1 .. 7 mod 8 once more with blocks of different sizes, n odd
    "n131": lambda: block_ranks(131, [10, 27, 44, 69, 94, 103], reverse_rows=(5, 80), far_rows=(120,)),
    # one block: every flag but entry 0 is set, M - 0 = M, five scans at start 0
    "n40-one-block": lambda: block_ranks(40, []),
    # a cut at 12, then one block of 48: >= 90 % at M = 48, 36, 24, 12, 0 - five scans, rows with L > M are NaN and count 1
    "n60-five-scans": lambda: block_ranks(60, [12]),
    # a cut at 20, then 27 of 30 flags: the ratio is .9 exactly (27.0 / 30.0 rounds to the literal's double)
    "n50-exactly-90%": lambda: block_ranks(50, [20], reverse_rows=(30, 40)),
    # a cut at 8, then counts significant at M = 72 and mostly not at M = 64: two scans at start 8
    "n80-two-scans": lambda: shrinking_ranks(80, 8, 72, 64),
    # the last block boundary at n - h (the last window whose right half is complete, h = 6) ...  (row 95 ranks the
    # other way round: with L = 47 of M = 48 its full count would be significant and spoil the clear half)
    "n96-last-window": lambda: block_ranks(96, [24, 48, 90], reverse_rows=(95,)),
    # ... and one position later, where the window scores 0
    "n96-past-last-window": lambda: block_ranks(96, [24, 48, 91], reverse_rows=(95,)),
    # stop_ind = 72 with min_frac .25: cuts at 72 (== stop_ind) / at 71 (stop_ind - 1, the loop goes on to 84)
    "n96-stop": lambda: block_ranks(96, [24, 48, 72, 84]),
    "n96-stop-1": lambda: block_ranks(96, [24, 48, 71, 84]),
    # n - ind == min_size (6) at the cut 90 and == min_size + 1 at the cut 89
    "n96-rest": lambda: block_ranks(96, [30, 60, 90], reverse_rows=(95,)),
    "n96-rest+1": lambda: block_ranks(96, [30, 60, 89]),
    # the decide workgroup strides by 1,024 lanes
    "n1024": lambda: block_ranks(1024, [300, 650, 1000], reverse_rows=(512,)),
    "n1025": lambda: block_ranks(1025, [301, 651, 1001], far_rows=(700,)),
    "n1100": lambda: block_ranks(1100, [202, 547, 1030, 1075]),
    # the threshold matrix of the grid (psig .05) under the loop's own count-and-flag kernel
    "n769-thresholds": lambda: mode0_ranks(.05),
    # filter maps
    "f120": lambda: block_ranks(120, [15, 33, 52, 70, 95], reverse_rows=(40,)),
    "f120-shared": lambda: shared_block_ranks(120, [20, 45, 64, 90], far_rows=(0, 1)),
    # MD = 420: rows 0 and 1 flag nothing, then blocks that end where a round's MD + 1 rows end, so every round is two scans
    "f2100": lambda: shared_block_ranks(2100, [2, 421, 841, 1261, 1681], far_rows=(0, 1)),
}

FirstPass = namedtuple("FirstPass", "name map min_size min_frac branch")
FIRST_PASS_CASES = [
    FirstPass("n2", "n2", 1, .05, "degenerate: one flag row"),
    FirstPass("n3", "n3", 1, .05, "degenerate"),
    FirstPass("n11", "n11", 2, .05, "degenerate: M <= 20, single-row counts are not significant"),
    FirstPass("n11-min-size-11", "n11", 11, .05, "min_size >= the rows left: NA NA NA, no cut"),
    FirstPass("n11-min-size-12", "n11", 12, .05, "min_size > n"),
    FirstPass("n77-h1", "n77-residues", 1, .05, "min_size = 1"),
    FirstPass("n77-h3", "n77-residues", 3, .05, "cuts at every residue of lo mod 8"),
    FirstPass("n77-h5-frac.3", "n77-residues", 5, .3, "stop_ind well inside the map"),
    FirstPass("n131-h4", "n131", 4, .05, "odd n, uneven blocks, rows that break the pattern"),
    FirstPass("n131-h9", "n131", 9, .05, "a block shorter than min_size + 1 is passed over"),
    FirstPass("n40-five-scans-same-M", "n40-one-block", 5, .05, ">= 90 % at start 0: M - 0 = M, five scans"),
    FirstPass("n60-five-scans-nan", "n60-five-scans", 5, .05, "five scans with a shrinking M; M - start < L: NaN rows count 1"),
    FirstPass("n50-exactly-90%", "n50-exactly-90%", 5, .05, "the flags' ratio equals .9: >= fires"),
    FirstPass("n80-two-scans", "n80-two-scans", 4, .05, ">= 90 % once, below it at the smaller M: stops before five"),
    FirstPass("n96-last-window", "n96-last-window", 6, .0, "cut in the last window whose right half is complete"),
    FirstPass("n96-past-last-window", "n96-past-last-window", 6, .0, "one position later: the window scores 0, no cut"),
    FirstPass("n96-ind==stop", "n96-stop", 5, .25, "ind == stop_ind ends the loop"),
    FirstPass("n96-ind==stop-1", "n96-stop-1", 5, .25, "ind == stop_ind - 1 goes on"),
    FirstPass("n96-rest==min_size", "n96-rest", 6, .0, "n - ind == min_size ends the loop"),
    FirstPass("n96-rest==min_size+1", "n96-rest+1", 6, .0, "n - ind == min_size + 1 goes on"),
    FirstPass("n1024", "n1024", 5, .05, "n == the decide workgroup's stride"),
    FirstPass("n1025", "n1025", 5, .05, "one row more than the stride"),
    FirstPass("n1100", "n1100", 7, .05, "a second lap of the stride"),
    FirstPass("n769-thresholds", "n769-thresholds", 1, .05, "every row's count within one of its threshold at start 0"),
]

Filter = namedtuple("Filter", "name map cuts psig branch")
_F120 = [15, 33, 52, 70, 95]
FILTER_CASES = [
    Filter("f120-one-candidate", "f120", (52,), .05, "a one-candidate list"),
    Filter("f120-true-cuts", "f120", tuple(_F120), .05, "the planted cuts: a restart at every candidate, local == 0 after it"),
    Filter("f120-true-cuts-.01", "f120", tuple(_F120), .01, "psig .01"),
    Filter("f120-true-cuts-1e-6", "f120", tuple(_F120), 1e-6, "psig 1e-6"),
    Filter("f120-noisy", "f120", (5, 15, 20, 33, 40, 52, 60, 70, 80, 95, 110), .05, "extra candidates inside the blocks"),
    Filter("f120-noisy-1e-6", "f120", (5, 15, 20, 33, 40, 52, 60, 70, 80, 95, 110), 1e-6, "psig 1e-6"),
    Filter("f120-dense", "f120", tuple(range(3, 118, 3)), .05, "every third index"),
    Filter("f120-dense-.01", "f120", tuple(range(2, 119, 2)), .01, "every second index, psig .01"),
    Filter("f120-far-candidates", "f120", (70, 95, 100, 110, 118), .05, "every candidate beyond MD: the MD + 1 row cap, no restart"),
    Filter("f120-zero", "f120", (0, 15, 33), .05, "candidate 0: local == 0 at start 0"),
    Filter("f120-shared-later-segment", "f120-shared", (3, 6, 9, 12, 20, 30, 45, 64, 90), .05,
           "noise in segments right of the scanned candidate: start jumps past it"),
    Filter("f120-shared-dense", "f120-shared", tuple(range(1, 119)), .05, "every index"),
    Filter("f120-shared-dense-1e-6", "f120-shared", tuple(range(1, 119, 2)), 1e-6, "psig 1e-6"),
    Filter("f2100-2047", "f2100", tuple(range(1, 2048)), .05, "one fewer than the LDS cap"),
    Filter("f2100-2048", "f2100", tuple(range(1, 2049)), .05, "the LDS cap exactly"),
    Filter("f2100-2049", "f2100", tuple(range(1, 2050)), .05, "one more: the first round walks its lists in global memory"),
]
# duplicate candidates cannot reach the device loop (hicmi_filter_cuts wants ascending indices; the package then keeps
# the per-scan host loop): host loop against the oracle only
DUPLICATE_CASES = [
    Filter("f120-duplicates", "f120", (15, 15, 33, 52, 52, 52, 70, 95, 95), .05, "duplicate candidates"),
    Filter("f120-shared-duplicates", "f120-shared", (3, 3, 6, 20, 20, 45, 64, 64, 90), .01, "duplicate candidates"),
]

FIRST_PASS_BY_NAME = {c.name: c for c in FIRST_PASS_CASES}
FILTER_BY_NAME = {c.name: c for c in FILTER_CASES + DUPLICATE_CASES}

FirstPassRef = namedtuple("FirstPassRef", "cuts mlog trace stop_ind")
FilterRef = namedtuple("FilterRef", "kept trace stats")


@functools.lru_cache(maxsize=None)
def first_pass_reference(name):
    import hic_oracle as ho
    case = FIRST_PASS_BY_NAME[name]
    trace = []
    cuts = ho.pre_process_all_matrix_breakpoints(ranks(case.map), min_size=case.min_size, min_frac=case.min_frac, trace=trace)
    # the M log: every scan whose flags reach 90 % changes M to M - start (S2C:473-477), the fifth of a start included
    mlog = [(int(e["M"]), int(e["M"] - e["start"])) for e in trace if int(e["sig"].sum()) / len(e["sig"]) >= .9]
    return FirstPassRef([int(v) for v in cuts], mlog, trace, stop_index(ranks(case.map).shape[0], case.min_frac))


@functools.lru_cache(maxsize=None)
def filter_reference(name):
    import hic_oracle as ho
    case = FILTER_BY_NAME[name]
    trace, stats = [], {}
    kept = ho.filter_noisy_breakpoints(ranks(case.map), list(case.cuts), psig=case.psig, trace=trace, stats=stats)
    return FilterRef([int(v) for v in kept], trace, stats)


def scans_per_start(trace):
    """[(start, [M of every scan at that start])] of a first-pass trace."""
    out = []
    for e in trace:
        if out and out[-1][0] == e["start"]:
            out[-1][1].append(int(e["M"]))
        else:
            out.append((int(e["start"]), [int(e["M"])]))
    return out
