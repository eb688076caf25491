"""NumPy restatement of DESIGN.md 9p - the read-pair links between the ends of ordered scaffolds - for the tests of
supportEnds: the ranks, the zones, the kind and the counter of every pair, the table by ``np.add.at``; a second,
brute-force table that loops over the pairs in plain Python integers; the per-scaffold and per-junction figures with their
verdicts; and a generator of an assembly with planted flips.  The assembly is laid out by ``liftmap_reference.layout``.
Nothing here calls the library or the package."""
import numpy as np

MAX_TABLE = 1 << 27
MAX_REACH = 64
COUNTERS = ("linked", "middle", "same", "too_far", "trans", "unlifted")
LINKED, MIDDLE, SAME, TOO_FAR, TRANS, UNLIFTED = range(6)
LEFT, RIGHT, MID = 0, 1, 2
LL, LR, RL, RR = 0, 1, 2, 3                                  # za * 2 + zb: zone at the lower rank, zone at the higher rank


# ---- ranks and zones -----------------------------------------------------------------------------------------------------
def number_ranks(sizes, tables):
    """(rank int32[S], seq_first int64[n_seq + 1], P): the placed scaffolds of size > 0, sequences ascending, inside a
    sequence by offset, then by index; -1 for a dropped or empty scaffold."""
    seq, off, _rev, seq_sizes = tables
    rank = np.full(len(sizes), -1, np.int32)
    seq_first = [0]
    n = 0
    for q in range(len(seq_sizes)):
        members = [s for s in range(len(sizes)) if seq[s] == q and sizes[s] > 0]
        for s in sorted(members, key=lambda s: (int(off[s]), s)):
            rank[s] = n
            n += 1
        seq_first.append(n)
    return rank, np.asarray(seq_first, np.int64), n


def fits(n_placed, reach):
    """Does the table of P x reach x 4 counters stay within the limit?"""
    return int(n_placed) * int(reach) * 4 <= MAX_TABLE


def zone_sizes(L, window):
    """(left zone, right zone) of a scaffold of L bases as it lies, in bases."""
    L, W = int(L), int(window)
    return min(W, L - L // 2), min(W, L // 2)


def zones(s, p, sizes, tables, window):
    """Zone of the 1-based positions ``p`` on the scaffolds ``s``: LEFT, RIGHT or MID."""
    _seq, _off, rev, _seq_sizes = tables
    s, p = np.asarray(s, np.int64), np.asarray(p, np.int64)
    L = np.asarray(sizes, np.int64)[s]
    W = np.int64(window)
    x = np.where(rev[s] != 0, L - p, p - 1)
    wl, wr = np.minimum(W, L - L // 2), np.minimum(W, L // 2)
    return np.where(x < wl, LEFT, np.where(x >= L - wr, RIGHT, MID))


# ---- the pairs ---------------------------------------------------------------------------------------------------------------
def classify(pairs, sizes, tables, window, reach):
    """(kind per pair as an index into COUNTERS, index of the counter in the flat table: -1 unless the pair is linked)."""
    seq, _off, _rev, _seq_sizes = tables
    rank, _seq_first, _n = number_ranks(sizes, tables)
    sa, pa, sb, pb = (np.asarray(x, np.int64) for x in pairs)
    R = int(reach)
    qa, qb = seq[sa].astype(np.int64), seq[sb].astype(np.int64)
    ra, rb = rank[sa].astype(np.int64), rank[sb].astype(np.int64)
    za, zb = zones(sa, pa, sizes, tables, window), zones(sb, pb, sizes, tables, window)
    d = np.abs(ra - rb)
    kind = np.zeros(len(sa), np.int64)
    kind[(za == MID) | (zb == MID)] = MIDDLE
    kind[d > R] = TOO_FAR
    kind[sa == sb] = SAME
    kind[qa != qb] = TRANS
    kind[(qa < 0) | (qb < 0)] = UNLIFTED
    a_low = ra < rb
    index = (np.minimum(ra, rb) * R + (d - 1)) * 4 + np.where(a_low, za * 2 + zb, zb * 2 + za)
    return kind, np.where(kind == LINKED, index, -1)


def table(pairs, sizes, tables, window, reach):
    """(T uint64[P, reach, 4], counters uint64[6])."""
    _rank, _seq_first, n = number_ranks(sizes, tables)
    assert 1 <= reach <= MAX_REACH and window >= 1 and n >= 1 and fits(n, reach)
    kind, index = classify(pairs, sizes, tables, window, reach)
    flat = np.zeros(n * int(reach) * 4, np.uint64)
    np.add.at(flat, index[kind == LINKED], np.uint64(1))
    return flat.reshape(n, int(reach), 4), np.bincount(kind, minlength=6).astype(np.uint64)


def brute_table(pairs, sizes, tables, window, reach):
    """The same straight from the definitions, pair by pair in Python integers."""
    seq, off, rev, seq_sizes = (np.asarray(x).tolist() for x in tables)
    sizes = [int(v) for v in sizes]
    order = sorted((s for s in range(len(sizes)) if seq[s] >= 0 and sizes[s] > 0), key=lambda s: (seq[s], off[s], s))
    rank = {s: i for i, s in enumerate(order)}
    T = [[[0, 0, 0, 0] for _d in range(reach)] for _i in order]
    counters = [0] * 6

    def zone(s, p):
        L = sizes[s]
        x = L - p if rev[s] else p - 1
        wl, wr = min(window, L - L // 2), min(window, L // 2)
        return LEFT if x < wl else RIGHT if x >= L - wr else MID

    for sa, pa, sb, pb in zip(*(np.asarray(x).tolist() for x in pairs)):
        assert 1 <= pa <= sizes[sa] and 1 <= pb <= sizes[sb]
        if seq[sa] < 0 or seq[sb] < 0:
            counters[UNLIFTED] += 1
        elif seq[sa] != seq[sb]:
            counters[TRANS] += 1
        elif sa == sb:
            counters[SAME] += 1
        elif abs(rank[sa] - rank[sb]) > reach:
            counters[TOO_FAR] += 1
        elif zone(sa, pa) == MID or zone(sb, pb) == MID:
            counters[MIDDLE] += 1
        else:
            counters[LINKED] += 1
            if rank[sa] > rank[sb]:
                sa, pa, sb, pb = sb, pb, sa, pa
            T[rank[sa]][rank[sb] - rank[sa] - 1][zone(sa, pa) * 2 + zone(sb, pb)] += 1
    return np.asarray(T, np.uint64).reshape(len(order), reach, 4), np.asarray(counters, np.uint64)


def outside(T, seq_first):
    """The entries of T whose i + d leaves the sequence of i: all of them must be 0."""
    P, R, _four = T.shape
    first = np.asarray(seq_first, np.int64)
    last = np.repeat(first[1:], np.diff(first))                   # per rank: the end of its sequence
    i, d = np.meshgrid(np.arange(P), np.arange(1, R + 1), indexing="ij")
    return T[(i + d) >= last[:, None]]


# ---- figures and verdicts ----------------------------------------------------------------------------------------------------
def scaffold_figures(T, seq_first, i):
    """(as_lies, flipped, alone) of the scaffold of rank i: the links its two ends have as it lies, and the ones they would
    have if it were turned round."""
    first = np.asarray(seq_first, np.int64)
    q = int(np.searchsorted(first, i, side="right")) - 1
    q0, q1 = int(first[q]), int(first[q + 1])
    R = T.shape[1]
    as_lies = flipped = 0
    for d in range(1, R + 1):
        if i + d < q1:
            as_lies += int(T[i, d - 1, RL])
            flipped += int(T[i, d - 1, LL])
        if i - d >= q0:
            as_lies += int(T[i - d, d - 1, RL])
            flipped += int(T[i - d, d - 1, RR])
    return as_lies, flipped, q1 - q0 == 1


def scaffold_verdict(as_lies, flipped, alone, min_pairs):
    if alone:
        return "NA"
    if as_lies + flipped < min_pairs or as_lies == flipped:
        return "open"
    return "supported" if as_lies > flipped else "flip"


def junction_figures(T, i):
    """(facing, left_flipped, right_flipped, both_flipped) of the junction between the ranks i and i + 1."""
    return int(T[i, 0, RL]), int(T[i, 0, LL]), int(T[i, 0, RR]), int(T[i, 0, LR])


def junction_verdict(figures, min_pairs):
    best = max(figures)
    if sum(figures) < min_pairs or list(figures).count(best) != 1:
        return "open"
    return ("held", "flip_left", "flip_right", "flip_both")[list(figures).index(best)]


# ---- an assembly with planted flips ------------------------------------------------------------------------------------------
PLANTED_WINDOW, PLANTED_REACH, PLANTED_MIN_PAIRS = 5000, 2, 4


def planted(seed=7, n_cis=60000, n_trans=2000):
    """A true genome of three chromosomes cut into 40 scaffolds, ten of them shorter than two windows, so that their zones are their halves; cis pairs with a
    heavy-tailed (log-uniform) distance in the coordinates of the true assembly plus uniform trans noise.  The truth is the
    order file ``true_chroms``; ``chroms`` is the one handed to the tool, in which the scaffolds ``flips`` have the wrong
    sign.  Read positions are those of the scaffolds' own + strands, which do not depend on either file.  Returns a dict
    with names, sizes, chroms, true_chroms, flips and pairs."""
    rng = np.random.default_rng(seed)
    lens = [[40000, 9000, 52000, 8000, 31000, 47000, 7500, 36000, 60000, 6200, 45000, 33000, 28000, 9900],
            [55000, 7000, 38000, 41000, 6700, 30000, 64000, 8500, 29000, 43000, 6500, 37000, 26000],
            [35000, 48000, 9000, 27000, 58000, 7200, 39000, 6600, 44000, 32000, 8000, 51000, 25000]]
    names, sizes, true_chroms, pieces = [], [], [], []
    g = 0
    for c, chrom in enumerate(lens):
        true_chroms.append([])
        for L in chrom:
            s = len(names)
            names.append("scaf_%d" % (s + 1))
            sizes.append(L)
            reversed_ = bool(rng.integers(0, 2))
            true_chroms[c].append((s, "-" if reversed_ else "+"))
            pieces.append((g, L, s, reversed_, c))
            g += L
    sizes = np.asarray(sizes, np.int64)
    assert len(names) == 40
    # the flips: long scaffolds and short ones (far below one bin of a 100 kb map), first and last ones of a chromosome
    flips = [0, 3, 9, 13, 15, 18, 26, 29, 34, 39]
    chroms = [[(s, ("+" if o == "-" else "-") if s in flips else o) for s, o in chrom] for chrom in true_chroms]
    p_start = np.array([t[0] for t in pieces])
    p_len = np.array([t[1] for t in pieces])
    p_rev = np.array([t[3] for t in pieces])
    p_chr = np.array([t[4] for t in pieces])
    chr_lo = np.array([p_start[p_chr == c].min() for c in range(3)])
    chr_hi = np.array([(p_start + p_len)[p_chr == c].max() for c in range(3)])

    def place(x):                                                # 0-based true coordinate -> (scaffold, 1-based position)
        k = np.searchsorted(p_start, x, side="right") - 1
        inside = x - p_start[k]
        return k.astype(np.int32), np.where(p_rev[k], p_len[k] - inside, inside + 1).astype(np.int64)

    weights = (chr_hi - chr_lo) / float((chr_hi - chr_lo).sum())
    c = rng.choice(3, n_cis, p=weights)
    a = chr_lo[c] + np.floor(rng.random(n_cis) * (chr_hi - chr_lo)[c]).astype(np.int64)
    d = np.exp(rng.uniform(np.log(100.0), np.log(100000.0), n_cis)).astype(np.int64) * rng.choice([-1, 1], n_cis)
    b = a + d
    ok = (b >= chr_lo[c]) & (b < chr_hi[c])
    xa = np.concatenate([a[ok], rng.integers(0, g, n_trans)])
    xb = np.concatenate([b[ok], rng.integers(0, g, n_trans)])
    mix = rng.permutation(len(xa))
    sa, pa = place(xa[mix])
    sb, pb = place(xb[mix])
    return {"names": names, "sizes": sizes, "chroms": chroms, "true_chroms": true_chroms, "flips": flips,
            "pairs": (sa, pa, sb, pb)}


def pair_file_bytes(names, pairs):
    """The pairs as an allValidPairs file."""
    sa, pa, sb, pb = (np.asarray(x).tolist() for x in pairs)
    return "".join("r%d\t%s\t%d\t+\t%s\t%d\t-\n" % (k, names[sa[k]], pa[k], names[sb[k]], pb[k]) for k in range(len(sa))).encode("ascii")
