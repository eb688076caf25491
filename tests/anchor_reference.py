"""NumPy restatement of DESIGN.md 9q - the read-pair links between the scaffolds an ordering leaves out and the placed
ones - for the tests of placeUnplaced: the blocks of the candidates, the kind and the counter of every pair, the table by
``np.add.at``; the choice of a chromosome with ``fractions.Fraction`` densities, the gap scores, the verdicts and the
``-placed`` text; and a generator of an assembly with scaffolds taken out.  The assembly is laid out by
``liftmap_reference.layout`` and ranked by ``ends_reference.number_ranks``.  Nothing here calls the library or the package."""
from fractions import Fraction

import numpy as np

import ends_reference as eref

MAX_TABLE = 1 << 27
COUNTERS = ("anchored", "middle", "elsewhere", "skipped", "unplaced", "placed")
ANCHORED, MIDDLE, ELSEWHERE, SKIPPED, UNPLACED, PLACED = range(6)
LEFT, RIGHT, MID = eref.LEFT, eref.RIGHT, eref.MID


# ---- blocks ------------------------------------------------------------------------------------------------------------------
def is_candidate(sizes, tables, target=None):
    seq = np.asarray(tables[0])
    sizes = np.asarray(sizes, np.int64)
    if target is None:
        return (seq == -1) & (sizes > 0)
    return np.asarray(target) >= 0


def number_blocks(sizes, tables, target=None):
    """(first int64[S], n_table): the candidates in index order, a block of n_seq counters each, or with ``target`` of
    4 x S_target; -1 for a non-candidate; n_table is -1 when the table passes MAX_TABLE."""
    n_seq = len(tables[3])
    _rank, seq_first, _n = eref.number_ranks(sizes, tables)
    first, n = [], 0
    for s, cand in enumerate(is_candidate(sizes, tables, target).tolist()):
        if not cand:
            first.append(-1)
            continue
        first.append(n)
        n += n_seq if target is None else 4 * int(seq_first[target[s] + 1] - seq_first[target[s]])
    return np.asarray(first, np.int64), (n if n <= MAX_TABLE else -1)


def halves(s, p, sizes):
    """The half of the candidates ``s`` the 1-based positions ``p`` fall in: 0 when p - 1 < len - len // 2, else 1."""
    L = np.asarray(sizes, np.int64)[np.asarray(s, np.int64)]
    return np.where(np.asarray(p, np.int64) - 1 < L - L // 2, 0, 1)


# ---- the pairs -----------------------------------------------------------------------------------------------------------------
def classify(pairs, sizes, tables, target, window):
    """(kind per pair as an index into COUNTERS, index of the counter in the table: -1 unless the pair is anchored)."""
    seq = np.asarray(tables[0], np.int64)
    rank, seq_first, _n = eref.number_ranks(sizes, tables)
    first, _total = number_blocks(sizes, tables, target)
    sa, pa, sb, pb = (np.asarray(x, np.int64) for x in pairs)
    a_lifts, b_lifts = seq[sa] >= 0, seq[sb] >= 0
    # u: the dropped end, v: the placed end (meaningless for the pairs that are placed or unplaced, which are set last)
    su, pu = np.where(a_lifts, sb, sa), np.where(a_lifts, pb, pa)
    sv, pv = np.where(a_lifts, sa, sb), np.where(a_lifts, pa, pb)
    q = seq[sv]
    kind = np.zeros(len(sa), np.int64)
    if target is None:
        index = first[su] + q
    else:
        tgt = np.asarray(target, np.int64)
        zp = eref.zones(sv, pv, sizes, tables, window)
        zu = halves(su, pu, sizes)
        index = first[su] + (rank[sv] - seq_first[np.maximum(q, 0)]) * 4 + zu * 2 + zp
        kind[zp == MID] = MIDDLE
        kind[tgt[su] != q] = ELSEWHERE
    kind[first[su] < 0] = SKIPPED
    kind[~a_lifts & ~b_lifts] = UNPLACED
    kind[a_lifts & b_lifts] = PLACED
    return kind, np.where(kind == ANCHORED, index, -1)


def table(pairs, sizes, tables, target, window):
    """(T uint64[n_table], counters uint64[6])."""
    _first, n = number_blocks(sizes, tables, target)
    assert window >= 1 and n >= 1
    kind, index = classify(pairs, sizes, tables, target, window)
    flat = np.zeros(n, np.uint64)
    np.add.at(flat, index[kind == ANCHORED], np.uint64(1))
    return flat, np.bincount(kind, minlength=6).astype(np.uint64)


def brute_table(pairs, sizes, tables, target, window):
    """The same straight from the definitions, pair by pair in Python integers."""
    seq, off, rev, seq_sizes = (np.asarray(x).tolist() for x in tables)
    sizes = [int(x) for x in sizes]
    n_seq = len(seq_sizes)
    members = [sorted((s for s in range(len(sizes)) if seq[s] == q and sizes[s] > 0), key=lambda s: (off[s], s)) for q in range(n_seq)]
    cands = [s for s in range(len(sizes)) if seq[s] < 0 and sizes[s] > 0 and (target is None or target[s] >= 0)]
    blocks, n = {}, 0
    for c in cands:
        blocks[c] = n
        n += n_seq if target is None else 4 * len(members[target[c]])
    T, counters = [0] * n, [0] * 6
    for sa, pa, sb, pb in zip(*(np.asarray(x).tolist() for x in pairs)):
        assert 1 <= pa <= sizes[sa] and 1 <= pb <= sizes[sb]
        if seq[sa] >= 0 and seq[sb] >= 0:
            counters[PLACED] += 1
            continue
        if seq[sa] < 0 and seq[sb] < 0:
            counters[UNPLACED] += 1
            continue
        (c, pc), (s, ps) = ((sa, pa), (sb, pb)) if seq[sa] < 0 else ((sb, pb), (sa, pa))
        if c not in blocks:
            counters[SKIPPED] += 1
        elif target is None:
            counters[ANCHORED] += 1
            T[blocks[c] + seq[s]] += 1
        elif seq[s] != target[c]:
            counters[ELSEWHERE] += 1
        else:
            L = sizes[s]
            x = L - ps if rev[s] else ps - 1
            zone = LEFT if x < min(window, L - L // 2) else RIGHT if x >= L - min(window, L // 2) else MID
            if zone == MID:
                counters[MIDDLE] += 1
                continue
            counters[ANCHORED] += 1
            half = 0 if pc - 1 < sizes[c] - sizes[c] // 2 else 1
            T[blocks[c] + members[seq[s]].index(s) * 4 + half * 2 + zone] += 1
    return np.asarray(T, np.uint64), np.asarray(counters, np.uint64)


# ---- decisions -----------------------------------------------------------------------------------------------------------------
def sequence_bases(sizes, tables):
    """B_q: the bases of the placed scaffolds of every sequence, gaps excluded."""
    seq = np.asarray(tables[0])
    return [int(np.asarray(sizes, np.int64)[seq == q].sum()) for q in range(len(tables[3]))]


def choose_chromosome(a, B, size, min_pairs, min_ratio, min_size):
    """(best, second, ratio, verdict or None): densities as exact fractions (a sequence without a base has the density 0:
    no pair can end on it)."""
    dens = [Fraction(int(x), int(b)) if b else Fraction(0) for x, b in zip(a, B)]
    by_density = sorted(range(len(a)), key=lambda q: (-dens[q], q))
    best = by_density[0]
    second = by_density[1] if len(a) > 1 else None
    ratio = None
    if second is not None:
        ratio = float("inf") if a[second] == 0 else (int(a[best]) * int(B[second])) / (int(a[second]) * int(B[best])) if a[best] else 0.0
    if size < min_size:
        verdict = "too_small"
    elif sum(int(x) for x in a) == 0:
        verdict = "no_links"
    elif a[best] < min_pairs or (second is not None and (dens[best] == dens[second] or ratio < min_ratio)):
        verdict = "ambiguous"
    else:
        verdict = None
    return best, second, ratio, verdict


def gap_scores(T, reach):
    """int scores[S + 1, 2] of every gap and the orientations + and - from T[k, zu, zp]."""
    S = T.shape[0]
    scores = np.zeros((S + 1, 2), dtype=object)
    for g in range(S + 1):
        lefts = [k for k in range(g - reach, g) if k >= 0]                # the scaffolds before the gap, their RIGHT zones
        rights = [k for k in range(g, g + reach) if k < S]               # the scaffolds after it, their LEFT zones
        scores[g, 0] = sum(int(T[k, 0, RIGHT]) for k in lefts) + sum(int(T[k, 1, LEFT]) for k in rights)
        scores[g, 1] = sum(int(T[k, 1, RIGHT]) for k in lefts) + sum(int(T[k, 0, LEFT]) for k in rights)
    return scores


def choose_gap(scores, min_pairs):
    """(gap, "+" / "-", m, runner_up, verdict)"""
    m = max(scores.reshape(-1).tolist())
    where = [(g, o) for g in range(scores.shape[0]) for o in (0, 1) if scores[g, o] == m]
    g, o = where[0]
    others = [scores[gg, oo] for gg in range(scores.shape[0]) for oo in (0, 1) if (gg, oo) != (g, o)]
    if m < min_pairs or len({gg for gg, _o in where}) > 1:
        verdict = "chromosome_only"
    else:
        verdict = "placed" if len(where) == 1 else "orientation_open"
    return g, "+-"[o], m, max(others), verdict


def place(sizes, chroms, pairs, window, reach, min_pairs, min_ratio, min_size, gap=100):
    """The whole decision on the reference's own tables: {candidate: dict(links, best, second, ratio, verdict, gap,
    orientation, score, runner_up)} and the winners {(chromosome, gap): candidate}."""
    import liftmap_reference as lref
    tables = lref.layout(chroms, sizes, gap, drop_unplaced=True)
    n_seq = len(chroms)
    B = sequence_bases(sizes, tables)
    first, _n = number_blocks(sizes, tables)
    T1, counters1 = table(pairs, sizes, tables, None, window)
    out, target = {}, np.full(len(sizes), -1, np.int32)
    for c in np.flatnonzero(first >= 0).tolist():
        a = [int(x) for x in T1[first[c]:first[c] + n_seq]]
        best, second, ratio, verdict = choose_chromosome(a, B, int(sizes[c]), min_pairs, min_ratio, min_size)
        out[c] = dict(links=a, best=best, second=second, ratio=ratio, verdict=verdict, gap=None, orientation=None, score=None, runner_up=None)
        if verdict is None:
            target[c] = best
    winners, counters2 = {}, np.zeros(6, np.uint64)
    if (target >= 0).any():
        first2, _n2 = number_blocks(sizes, tables, target)
        T2, counters2 = table(pairs, sizes, tables, target, window)
        _rank, seq_first, _p = eref.number_ranks(sizes, tables)
        for c in np.flatnonzero(target >= 0).tolist():
            S = int(seq_first[target[c] + 1] - seq_first[target[c]])
            scores = gap_scores(T2[first2[c]:first2[c] + 4 * S].reshape(S, 2, 2), reach)
            g, o, m, runner_up, verdict = choose_gap(scores, min_pairs)
            out[c].update(gap=g, orientation=o, score=m, runner_up=runner_up, verdict=verdict, scores=scores)
        for c in sorted(out):
            if out[c]["verdict"] in ("placed", "orientation_open"):
                key = (out[c]["best"], out[c]["gap"])
                if key not in winners or out[c]["score"] > out[winners[key]]["score"]:
                    winners[key] = c
        for c in out:
            if out[c]["verdict"] in ("placed", "orientation_open") and winners[(out[c]["best"], out[c]["gap"])] != c:
                out[c]["verdict"] = "deferred"
    return out, winners, counters1, counters2


def placed_text(order_text, names, sizes, chroms, result, winners):
    """The ``-placed`` file: ``order_text`` with the winners inserted."""
    lines = order_text.splitlines(keepends=True)
    at = {}                                                               # scaffold name -> line number
    for k, line in enumerate(lines):
        body = line.rstrip("\r\n")
        if k and body and not body.startswith("#"):
            at[body.split("\t")[0]] = k
    before, after = {}, {}
    for (q, g), c in winners.items():
        members = [s for s, _o in chroms[q] if sizes[s] > 0]
        text = "%s\t%s" % (names[c], result[c]["orientation"])
        if g < len(members):
            before[at[names[members[g]]]] = text
        else:
            after[at[names[members[-1]]]] = text
    out = []
    for k, line in enumerate(lines):
        body = line.rstrip("\r\n")
        ending = line[len(body):]
        if k in before:
            out.append(before[k] + (ending or "\n"))
        if k in after and not ending:
            out += [body + "\n", after[k]]
            continue
        out.append(line)
        if k in after:
            out.append(after[k] + ending)
    return "".join(out)


# ---- an assembly with scaffolds taken out ------------------------------------------------------------------------------------
PLANTED_WINDOW, PLANTED_REACH, PLANTED_MIN_PAIRS, PLANTED_MIN_RATIO = 5000, 2, 4, 2.0
PLANTED_REMOVED = [0, 3, 9, 13, 26, 29, 30, 39]


def planted():
    """The genome of ``ends_reference.planted`` - three chromosomes, 40 scaffolds, cis pairs with a log-uniform distance plus
    trans noise - in its true order, with eight scaffolds taken out of the order file: 6.2 to 60 kb, a chromosome's first
    (scaf_1) and its last (scaf_14, scaf_27, scaf_40), ``+`` and ``-`` ones, and two neighbours (scaf_30, scaf_31), which
    belong in one gap.  Returns a dict with names, sizes, true_chroms, chroms (without the removed ones), removed and pairs."""
    P = eref.planted()
    removed = list(PLANTED_REMOVED)
    chroms = [[(s, o) for s, o in chrom if s not in removed] for chrom in P["true_chroms"]]
    return {"names": P["names"], "sizes": P["sizes"], "true_chroms": P["true_chroms"], "chroms": chroms, "removed": removed,
            "pairs": P["pairs"]}


def planted_truth(P, chroms=None):
    """{removed scaffold: (chromosome, gap among the scaffolds of ``chroms``, orientation)} from the true layout."""
    chroms = P["chroms"] if chroms is None else chroms
    truth = {}
    for q, chrom in enumerate(P["true_chroms"]):
        present = {s for s, _o in chroms[q]}
        g = 0
        for s, o in chrom:
            if s in present:
                g += 1
            elif s in P["removed"]:
                truth[s] = (q, g, o)
    return truth


def pair_file_bytes(names, pairs):
    return eref.pair_file_bytes(names, pairs)
