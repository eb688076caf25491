"""NumPy restatement of DESIGN.md 9s - seat support, every placed scaffold taken out and re-placed from its read pairs -
for the tests of supportSeats and of polishOrder's relocate rounds: the blocks of the placed scaffolds, the kind and the up
to four counters of every pair, the table by ``np.add.at``; a second, brute-force table that loops over the pairs in plain
Python integers; the table and the counters from a resident store; and the layout with one scaffold left out.  The
assembly is ranked by ``ends_reference.number_ranks``.  Nothing here calls the library or the package."""
import numpy as np

import ends_reference as eref

MAX_TABLE = 1 << 27
COUNTERS = ("seated", "middle", "trans", "same", "unlifted")
SEATED, MIDDLE, TRANS, SAME, UNLIFTED = range(5)
NOWHERE = -1
LEFT, RIGHT, MID = eref.LEFT, eref.RIGHT, eref.MID


# ---- blocks --------------------------------------------------------------------------------------------------------------------
def number_blocks(sizes, tables):
    """(first int64[S], n_table): the placed scaffolds with a base in index order, a block of n_seq + 4 x S_q counters each;
    -1 for a dropped or empty scaffold; n_table is -1 when the table passes MAX_TABLE."""
    seq = np.asarray(tables[0]).tolist()
    n_seq = len(tables[3])
    rank, seq_first, _n = eref.number_ranks(sizes, tables)
    first, n = [], 0
    for s in range(len(sizes)):
        if rank[s] < 0:
            first.append(-1)
            continue
        first.append(n)
        n += n_seq + 4 * int(seq_first[seq[s] + 1] - seq_first[seq[s]])
    return np.asarray(first, np.int64), (n if n <= MAX_TABLE else -1)


def halves(s, p, sizes):
    """The half of the scaffolds ``s`` the 1-based positions ``p`` fall in: 0 when p - 1 < len - len // 2, else 1."""
    L = np.asarray(sizes, np.int64)[np.asarray(s, np.int64)]
    return np.where(np.asarray(p, np.int64) - 1 < L - L // 2, 0, 1)


# ---- the pairs -----------------------------------------------------------------------------------------------------------------
def classify(pairs, sizes, tables, window):
    """(kind per pair as an index into COUNTERS, index int64[n, 4] of the counters it adds to, -1 for the unused ones, in the
    order chromosome of a, chromosome of b, gap of a, gap of b with the used ones first)."""
    seq = np.asarray(tables[0], np.int64)
    n_seq = len(tables[3])
    rank, seq_first, _n = eref.number_ranks(sizes, tables)
    rank = rank.astype(np.int64)
    first, _total = number_blocks(sizes, tables)
    sa, pa, sb, pb = (np.asarray(x, np.int64) for x in pairs)
    qa, qb = seq[sa], seq[sb]
    lifted = (qa >= 0) & (qb >= 0)
    between = lifted & (sa != sb)
    cis = between & (qa == qb)
    za, zb = eref.zones(sa, pa, sizes, tables, window), eref.zones(sb, pb, sizes, tables, window)
    ha, hb = halves(sa, pa, sizes), halves(sb, pb, sizes)
    q0 = seq_first[np.maximum(qa, 0)]
    gap_a = first[sa] + n_seq + (rank[sb] - q0) * 4 + ha * 2 + zb        # a's block: the other end lies on b
    gap_b = first[sb] + n_seq + (rank[sa] - q0) * 4 + hb * 2 + za
    use_a, use_b = cis & (zb != MID), cis & (za != MID)
    index = np.full((len(sa), 4), -1, np.int64)
    index[between, 0] = (first[sa] + qb)[between]
    index[between, 1] = (first[sb] + qa)[between]
    index[use_a, 2] = gap_a[use_a]
    only_b = use_b & ~use_a
    index[only_b, 2] = gap_b[only_b]
    both = use_a & use_b
    index[both, 3] = gap_b[both]
    kind = np.full(len(sa), MIDDLE, np.int64)
    kind[use_a | use_b] = SEATED
    kind[between & (qa != qb)] = TRANS
    kind[lifted & (sa == sb)] = SAME
    kind[~lifted] = UNLIFTED
    return kind, index


def table(pairs, sizes, tables, window):
    """(T uint64[n_table], counters uint64[5])."""
    _first, n = number_blocks(sizes, tables)
    assert window >= 1 and n >= 1
    kind, index = classify(pairs, sizes, tables, window)
    flat = np.zeros(n, np.uint64)
    np.add.at(flat, index[index >= 0], np.uint64(1))
    return flat, np.bincount(kind, minlength=5).astype(np.uint64)


def brute_table(pairs, sizes, tables, window):
    """The same straight from the definitions, pair by pair in Python integers."""
    seq, off, rev, seq_sizes = (np.asarray(x).tolist() for x in tables)
    sizes = [int(x) for x in sizes]
    n_seq = len(seq_sizes)
    members = [sorted((s for s in range(len(sizes)) if seq[s] == q and sizes[s] > 0), key=lambda s: (off[s], s)) for q in range(n_seq)]
    blocks, n = {}, 0
    for s in range(len(sizes)):
        if seq[s] >= 0 and sizes[s] > 0:
            blocks[s] = n
            n += n_seq + 4 * len(members[seq[s]])
    T, counters = [0] * n, [0] * 5

    def zone(s, p):
        L = sizes[s]
        x = L - p if rev[s] else p - 1
        return LEFT if x < min(window, L - L // 2) else RIGHT if x >= L - min(window, L // 2) else MID

    def half(s, p):
        return 0 if p - 1 < sizes[s] - sizes[s] // 2 else 1

    for sa, pa, sb, pb in zip(*(np.asarray(x).tolist() for x in pairs)):
        assert 1 <= pa <= sizes[sa] and 1 <= pb <= sizes[sb]
        if seq[sa] < 0 or seq[sb] < 0:
            counters[UNLIFTED] += 1
            continue
        if sa == sb:
            counters[SAME] += 1
            continue
        T[blocks[sa] + seq[sb]] += 1
        T[blocks[sb] + seq[sa]] += 1
        if seq[sa] != seq[sb]:
            counters[TRANS] += 1
            continue
        seated = False
        for (c, pc), (s, ps) in (((sa, pa), (sb, pb)), ((sb, pb), (sa, pa))):
            z = zone(s, ps)
            if z != MID:
                T[blocks[c] + n_seq + members[seq[s]].index(s) * 4 + half(c, pc) * 2 + z] += 1
                seated = True
        counters[SEATED if seated else MIDDLE] += 1
    return np.asarray(T, np.uint64), np.asarray(counters, np.uint64)


def store_table(kept, intra_counts, sizes, tables, window):
    """(table, counters) of 9s from a resident store (pairs_reference): the kept pairs counted, the intra pairs added as
    ``same`` and ``unlifted``."""
    T, counters = table(kept, sizes, tables, window)
    placed = np.asarray(tables[0]) >= 0
    counters = counters.copy()
    counters[SAME] += np.uint64(int(intra_counts[placed].sum()))
    counters[UNLIFTED] += np.uint64(int(intra_counts[~placed].sum()))
    return T, counters


# ---- one scaffold left out -------------------------------------------------------------------------------------------------------
def without(tables, c):
    """The lift tables with the scaffold ``c`` alone dropped; every other scaffold lies where it lay."""
    seq, off, rev, seq_sizes = (np.array(x) for x in tables)
    seq[c] = -1
    return seq, off, rev, seq_sizes


def own_block(T, first, sizes, tables, c):
    """(a int[n_seq], gaps uint64[S_q, 2, 2], k_c) of the placed scaffold ``c``."""
    n_seq = len(tables[3])
    rank, seq_first, _n = eref.number_ranks(sizes, tables)
    q = int(tables[0][c])
    S = int(seq_first[q + 1] - seq_first[q])
    at = int(first[c])
    return T[at:at + n_seq], T[at + n_seq:at + n_seq + 4 * S].reshape(S, 2, 2), int(rank[c] - seq_first[q])
