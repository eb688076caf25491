"""NumPy restatement of DESIGN.md 9r - the resident pair store - for the tests of the store and of polishOrder: the kept
mask, ``intra`` by ``bincount``, the tables of 9p and 9q computed from (kept pairs, intra) through ``ends_reference`` and
``anchor_reference``, and a stand-in context that answers the resident calls from them.  Nothing here calls the library or
the package."""
import numpy as np

import anchor_reference as aref
import buildmap_reference as bref
import ends_reference as eref


def as_pairs(pairs):
    sa, pa, sb, pb = pairs
    return (np.asarray(sa, np.int32), np.asarray(pa, np.int64), np.asarray(sb, np.int32), np.asarray(pb, np.int64))


def mask(pairs):
    """True for the pairs the store keeps: the ends lie on two scaffolds."""
    sa, _pa, sb, _pb = as_pairs(pairs)
    return sa != sb


def keep(pairs):
    """The store after these pairs: the NumPy boolean mask of the input, in the order it came."""
    m = mask(pairs)
    return tuple(x[m] for x in as_pairs(pairs))


def intra(pairs, n_scaf):
    """intra uint64[n_scaf]: the pairs with both ends on one scaffold, per scaffold."""
    sa = as_pairs(pairs)[0]
    return np.bincount(sa[~mask(pairs)], minlength=n_scaf).astype(np.uint64)


def intra_sums(intra_counts, lift_seq):
    """(on placed scaffolds, on dropped scaffolds)."""
    placed = np.asarray(lift_seq) >= 0
    return int(intra_counts[placed].sum()), int(intra_counts[~placed].sum())


def sorted_rows(pairs):
    """The pairs as rows in a fixed order: what the plain form's store is compared by."""
    rows = np.stack([np.asarray(x, np.int64) for x in pairs], axis=1) if len(pairs[0]) else np.zeros((0, 4), np.int64)
    return rows[np.lexsort(rows.T[::-1])]


def ends_table(kept, intra_counts, sizes, tables, window, reach):
    """(T, counters) of 9p from the store: the kept pairs counted, the intra pairs added as ``same`` and ``unlifted``."""
    T, counters = eref.table(kept, sizes, tables, window, reach)
    placed, dropped = intra_sums(intra_counts, tables[0])
    counters = counters.copy()
    counters[eref.SAME] += np.uint64(placed)
    counters[eref.UNLIFTED] += np.uint64(dropped)
    return T, counters


def anchor_table(kept, intra_counts, sizes, tables, target, window):
    """(table, counters) of 9q from the store: the intra pairs added as ``placed`` and ``unplaced``."""
    T, counters = aref.table(kept, sizes, tables, target, window)
    placed, dropped = intra_sums(intra_counts, tables[0])
    counters = counters.copy()
    counters[aref.COUNTERS.index("placed")] += np.uint64(placed)
    counters[aref.COUNTERS.index("unplaced")] += np.uint64(dropped)
    return T, counters


class StandInContext:
    """The store calls of _lib.Context that polishOrder uses, answered by the reference."""

    def __init__(self):
        self.calls, self.store = [], None

    def pairs_file(self, path, names, sizes, threads=0):
        assert self.store is None, "the context already has a store"
        with open(path, "rb") as fh:
            pairs, stats, _after = bref.parse_text(fh.read(), names, sizes)
        self.store = (keep(pairs), intra(pairs, len(sizes)), np.asarray(sizes, np.int64))
        self.calls.append("pairs_file")
        return tuple(stats) + (1,)

    def pairs_info(self):
        kept, counts, _sizes = self.store
        return len(kept[0]), int(counts.sum()), counts.copy()

    def pairs_drop(self):
        assert self.store is not None
        self.store = None
        self.calls.append("pairs_drop")

    @staticmethod
    def _tables(lift_seq, lift_off, lift_rev, seq_sizes):
        return (np.asarray(lift_seq, np.int32), np.asarray(lift_off, np.int64), np.asarray(lift_rev, np.uint8), np.asarray(seq_sizes, np.int64))

    def ends_resident(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, window, reach):
        kept, counts, store_sizes = self.store
        assert np.array_equal(store_sizes, np.asarray(sizes, np.int64))
        tables = self._tables(lift_seq, lift_off, lift_rev, seq_sizes)
        T, counters = ends_table(kept, counts, store_sizes, tables, window, reach)
        self.calls.append("ends_resident")
        return eref.number_ranks(store_sizes, tables)[0], T, counters

    def anchor_resident(self, sizes, lift_seq, lift_off, lift_rev, seq_sizes, target, window):
        kept, counts, store_sizes = self.store
        assert np.array_equal(store_sizes, np.asarray(sizes, np.int64))
        tables = self._tables(lift_seq, lift_off, lift_rev, seq_sizes)
        tgt = None if target is None else np.asarray(target, np.int32)
        T, counters = anchor_table(kept, counts, store_sizes, tables, tgt, window)
        self.calls.append("anchor_resident")
        return aref.number_blocks(store_sizes, tables, tgt)[0], T, counters
