"""NumPy restatement of DESIGN.md 9t - the end-link graph of all scaffolds - for the tests of scaffoldLinks: the zone of a
read end on a scaffold in its own + coordinates, the combination and the 64-bit key of a pair, the rows by ``np.unique`` and
the two counters; a second, brute-force version that loops over the pairs in plain Python integers; the capacity rule; and a
stand-in context that answers ``links_resident`` from a ``pairs_reference`` store.  Nothing here calls the library or the
package."""
import numpy as np

import ends_reference as eref
import pairs_reference as pref

LL, LR, RL, RR, OTHER = range(5)
COUNTERS = ("linked", "middle")
LINKED, MIDDLE = 0, 1
LEFT, RIGHT, MID = eref.LEFT, eref.RIGHT, eref.MID
MAX_SCAF, MIN_SLOTS, MAX_SLOTS = 1 << 30, 1024, 1 << 31
EMPTY = (1 << 64) - 1


def zones(s, p, sizes, window):
    """Zone of the 1-based positions ``p`` on the scaffolds ``s``, every scaffold read left to right as the size file has it."""
    s, p = np.asarray(s, np.int64), np.asarray(p, np.int64)
    L = np.asarray(sizes, np.int64)[s]
    W = np.int64(window)
    x = p - 1
    return np.where(x < np.minimum(W, L - L // 2), LEFT, np.where(x >= L - np.minimum(W, L // 2), RIGHT, MID))


def classify(pairs, sizes, window):
    """(lo, hi, combination, key uint64) per pair of a store: every pair lies on two scaffolds."""
    sa, pa, sb, pb = (np.asarray(x, np.int64) for x in pairs)
    assert np.all(sa != sb)
    za, zb = zones(sa, pa, sizes, window), zones(sb, pb, sizes, window)
    a_low = sa < sb
    lo, hi = np.where(a_low, sa, sb), np.where(a_low, sb, sa)
    zlo, zhi = np.where(a_low, za, zb), np.where(a_low, zb, za)
    combo = np.where((zlo == MID) | (zhi == MID), OTHER, zlo * 2 + zhi)
    key = (lo.astype(np.uint64) << np.uint64(33)) | (hi.astype(np.uint64) << np.uint64(3)) | combo.astype(np.uint64)
    return lo, hi, combo, key


def rows(pairs, sizes, window):
    """(lo int32[E], hi int32[E], counts uint64[E, 5], counters uint64[2]): one row per scaffold pair with a pair, sorted by
    (lo, hi)."""
    lo, hi, combo, _key = classify(pairs, sizes, window)
    S = len(sizes)
    pair_id, inverse = np.unique(lo * S + hi, return_inverse=True)
    counts = np.zeros((len(pair_id), 5), np.uint64)
    np.add.at(counts, (inverse.reshape(-1), combo), np.uint64(1))
    counters = np.asarray([int((combo != OTHER).sum()), int((combo == OTHER).sum())], np.uint64)
    return (pair_id // S).astype(np.int32), (pair_id % S).astype(np.int32), counts, counters


def brute_rows(pairs, sizes, window):
    """The same straight from the definitions, pair by pair in Python integers."""
    sizes = [int(v) for v in sizes]
    table, counters = {}, [0, 0]

    def zone(s, p):
        L = sizes[s]
        left, right = min(window, L - L // 2), min(window, L // 2)
        return LEFT if p - 1 < left else RIGHT if p - 1 >= L - right else MID

    for sa, pa, sb, pb in zip(*(np.asarray(x).tolist() for x in pairs)):
        assert sa != sb and 1 <= pa <= sizes[sa] and 1 <= pb <= sizes[sb]
        if sa > sb:
            sa, pa, sb, pb = sb, pb, sa, pa
        za, zb = zone(sa, pa), zone(sb, pb)
        combo = OTHER if MID in (za, zb) else za * 2 + zb
        table.setdefault((sa, sb), [0] * 5)[combo] += 1
        counters[MIDDLE if combo == OTHER else LINKED] += 1
    keys = sorted(table)
    return (np.asarray([k[0] for k in keys], np.int32), np.asarray([k[1] for k in keys], np.int32),
            np.asarray([table[k] for k in keys], np.uint64).reshape(len(keys), 5), np.asarray(counters, np.uint64))


def key_of(lo, hi, combo):
    return int(lo) << 33 | int(hi) << 3 | int(combo)


def slot_of(key, bits):
    """The slot a key starts probing at in a table of 2**bits slots."""
    return ((int(key) * 0x9E3779B97F4A7C15) & EMPTY) >> (64 - bits)


def capacity(n_kept, n_scaf):
    """The smallest power of two that is at least 1,024 and at least twice min(n_kept, 5 n_scaf (n_scaf - 1) / 2), in
    Python integers."""
    most = min(int(n_kept), 5 * int(n_scaf) * (int(n_scaf) - 1) // 2) if n_kept > 0 and n_scaf > 1 else 0
    cap = MIN_SLOTS
    while cap < 2 * most:
        cap *= 2
    return cap


class StandInContext(pref.StandInContext):
    """``pairs_reference.StandInContext`` with ``links_resident`` answered by this reference."""

    def links_resident(self, sizes, window):
        kept, _counts, store_sizes = self.store
        assert np.array_equal(store_sizes, np.asarray(sizes, np.int64)) and window >= 1
        self.calls.append("links_resident")
        if len(kept[0]) == 0:
            return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 5), np.uint64), np.zeros(2, np.uint64)
        return rows(kept, store_sizes, window)
