"""NumPy restatement of DESIGN.md 9u - the end-link graph between the ends of sequences that consist of several scaffolds -
for the tests of ``links_lifted`` and of scaffoldLinks -rounds: both ends of a pair lifted onto their sequences, the zone of
a lifted end on its sequence read left to right, the combination and the 64-bit key of the two sequences, the rows by
``np.unique`` and the four counters; a second, brute-force version that loops over the pairs in plain Python integers; the
tables of a layout of sequences; and a stand-in context that answers ``links_lifted`` from a ``pairs_reference`` store.
Nothing here calls the library or the package."""
import numpy as np

import links_reference as lref

COUNTERS = ("linked", "middle", "inside", "unlifted")
LINKED, MIDDLE, INSIDE, UNLIFTED = range(4)
NO_ROWS = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 5), np.uint64))


def tables_of(sequences, sizes, gap):
    """(lift_seq, lift_off, lift_rev, seq_sizes) of ``sequences`` - lists of (scaffold index, "+" / "-") - laid out from
    offset 0 with ``gap`` bases between neighbours; a scaffold no sequence names is dropped (-1)."""
    S = len(sizes)
    seq, off, rev, seq_sizes = np.full(S, -1, np.int32), np.zeros(S, np.int64), np.zeros(S, np.uint8), []
    for q, members in enumerate(sequences):
        at = 0
        for k, (s, o) in enumerate(members):
            assert seq[s] == -1 and o in ("+", "-")
            at += gap if k else 0
            seq[s], off[s], rev[s] = q, at, o == "-"
            at += int(sizes[s])
        seq_sizes.append(at)
    return seq, off, rev, np.asarray(seq_sizes, np.int64)


def rows(pairs, sizes, tables, window):
    """(lo int32[E], hi int32[E], counts uint64[E, 5], counters uint64[4]): one row per pair of sequences with a pair between
    them, sorted by (lo, hi)."""
    seq, off, rev, seq_sizes = (np.asarray(x, np.int64) for x in tables)
    sa, pa, sb, pb = (np.asarray(x, np.int64) for x in pairs)
    assert np.all(sa != sb)
    L = np.asarray(sizes, np.int64)
    qa, qb = seq[sa], seq[sb]
    lifted = (qa >= 0) & (qb >= 0)
    between = lifted & (qa != qb)
    counters = [0, 0, int((lifted & (qa == qb)).sum()), int((~lifted).sum())]
    sa, pa, sb, pb, qa, qb = (x[between] for x in (sa, pa, sb, pb, qa, qb))
    if len(sa) == 0:
        return NO_ROWS + (np.asarray(counters, np.uint64),)
    ya = off[sa] + np.where(rev[sa] != 0, L[sa] - pa + 1, pa)
    yb = off[sb] + np.where(rev[sb] != 0, L[sb] - pb + 1, pb)
    # from here on the sequences are the scaffolds of 9t and the lifted positions the positions on them
    lo, hi, counts, two = lref.rows((qa, ya, qb, yb), seq_sizes, window)
    counters[LINKED], counters[MIDDLE] = int(two[0]), int(two[1])
    return lo, hi, counts, np.asarray(counters, np.uint64)


def brute_classify(sizes, tables, window, sa, pa, sb, pb):
    """(kind, key) of one pair straight from the definitions, in Python integers; the key is 0 for inside and unlifted."""
    seq, off, rev, seq_sizes = tables
    ends = []
    for s, p in ((int(sa), int(pa)), (int(sb), int(pb))):
        size = int(sizes[s])
        assert 1 <= p <= size
        if int(seq[s]) < 0:
            return UNLIFTED, 0
        ends.append((int(seq[s]), int(off[s]) + (size - p + 1 if int(rev[s]) else p)))
    (qa, ya), (qb, yb) = ends
    if qa == qb:
        return INSIDE, 0

    def zone(q, y):
        size = int(seq_sizes[q])
        assert 1 <= y <= size
        left, right = min(window, size - size // 2), min(window, size // 2)
        return lref.LEFT if y - 1 < left else lref.RIGHT if y - 1 >= size - right else lref.MID

    if qa > qb:
        qa, ya, qb, yb = qb, yb, qa, ya
    za, zb = zone(qa, ya), zone(qb, yb)
    combo = lref.OTHER if lref.MID in (za, zb) else za * 2 + zb
    return (MIDDLE if combo == lref.OTHER else LINKED), lref.key_of(qa, qb, combo)


def brute_rows(pairs, sizes, tables, window):
    """The rows and the counters pair by pair."""
    table, counters = {}, [0] * 4
    for sa, pa, sb, pb in zip(*(np.asarray(x).tolist() for x in pairs)):
        assert sa != sb
        kind, key = brute_classify(sizes, tables, window, sa, pa, sb, pb)
        counters[kind] += 1
        if kind in (LINKED, MIDDLE):
            table.setdefault((key >> 33, (key >> 3) & ((1 << 30) - 1)), [0] * 5)[key & 7] += 1
    keys = sorted(table)
    return (np.asarray([k[0] for k in keys], np.int32), np.asarray([k[1] for k in keys], np.int32),
            np.asarray([table[k] for k in keys], np.uint64).reshape(len(keys), 5), np.asarray(counters, np.uint64))


class StandInContext(lref.StandInContext):
    """``links_reference.StandInContext`` with ``links_lifted`` answered by this reference."""

    def links_lifted(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window):
        kept, _counts, store_sizes = self.store
        assert np.array_equal(store_sizes, np.asarray(sizes, np.int64)) and window >= 1
        self.calls.append("links_lifted")
        tables = self._tables(lift_seq, lift_off, lift_rev, seq_sizes)
        if len(kept[0]) == 0:
            return NO_ROWS + (np.zeros(4, np.uint64),)
        return rows(kept, store_sizes, tables, window)
