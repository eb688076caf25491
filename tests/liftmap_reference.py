"""Plain-Python restatement of DESIGN.md 9m - read pairs lifted from scaffolds onto the sequences of an assembly, the
map counted there, the cis / trans split and the contact-decay histogram - for the tests of assembledMap.  The lift and
the statistics are Python integers (``int.bit_length()`` for the slot); the lifted pairs then go to
``buildmap_reference.build`` on the sequence sizes.  Nothing here calls the library or the package."""
import numpy as np

import buildmap_reference as bref

R = bref.R
SLOTS = 256


def layout(chromosomes, sizes, gap, drop_unplaced=False):
    """(lift_seq, lift_off, lift_rev, seq_sizes) for ``chromosomes`` - lists of (scaffold index, "+" / "-") - over scaffolds
    of the sizes ``sizes``: scaffold k of a chromosome starts at sum_{q<k} (L_q + gap); every scaffold no chromosome names
    follows as a sequence of its own, in index order, or is dropped (-1)."""
    S = len(sizes)
    seq, off, rev = [-1] * S, [0] * S, [0] * S
    seq_sizes = []
    for c, chrom in enumerate(chromosomes):
        at = 0
        for k, (s, o) in enumerate(chrom):
            assert seq[s] == -1 and o in "+-"
            if k:
                at += gap
            seq[s], off[s], rev[s] = c, at, int(o == "-")
            at += int(sizes[s])
        seq_sizes.append(at)
    if not drop_unplaced:
        for s in range(S):
            if seq[s] == -1:
                seq[s] = len(seq_sizes)
                seq_sizes.append(int(sizes[s]))
    return (np.asarray(seq, np.int32), np.asarray(off, np.int64), np.asarray(rev, np.uint8), np.asarray(seq_sizes, np.int64))


def identity(sizes):
    """Every scaffold its own + sequence, in order."""
    return layout([], sizes, 0)


def lift_one(tables, sizes, s, p):
    """(sequence, position) of the 1-based position p on scaffold s; (-1, 0) on a dropped scaffold."""
    seq, off, rev, _seq_sizes = tables
    s, p, L = int(s), int(p), int(sizes[s])
    assert 1 <= p <= L
    if seq[s] < 0:
        return -1, 0
    return int(seq[s]), int(off[s]) + (L - p + 1 if rev[s] else p)


def slot(d):
    """Slot of the distance d: 0 for 0, else 1 + 4 e + (((d - 2^e) * 4) >> e) with e = floor(log2 d)."""
    d = int(d)
    if d == 0:
        return 0
    e = d.bit_length() - 1
    return 1 + 4 * e + (((d - (1 << e)) * 4) >> e)


def lift_and_stats(pairs, sizes, tables):
    """The lifted pairs (sequence a, position a, sequence b, position b) without the unlifted ones, and
    (decay[256], seq_cis, seq_trans, unlifted) as Python-integer lists."""
    n_seq = len(tables[3])
    decay, cis, trans, unlifted = [0] * SLOTS, [0] * n_seq, [0] * n_seq, 0
    out = []
    for sa, pa, sb, pb in zip(*(np.asarray(x).tolist() for x in pairs)):
        qa, xa = lift_one(tables, sizes, sa, pa)
        qb, xb = lift_one(tables, sizes, sb, pb)
        if qa < 0 or qb < 0:
            unlifted += 1
            continue
        out.append((qa, xa, qb, xb))
        if qa == qb:
            cis[qa] += 1
            decay[slot(abs(xa - xb))] += 1
        else:
            trans[qa] += 1
            trans[qb] += 1
    arr = np.asarray(out, dtype=np.int64).reshape(-1, 4)
    lifted = (arr[:, 0].astype(np.int32), arr[:, 1].copy(), arr[:, 2].astype(np.int32), arr[:, 3].copy())
    return lifted, (decay, cis, trans, unlifted)


def build(pairs, sizes, tables, r):
    """(the dense lifted map at bin size r, the statistics)."""
    lifted, stats = lift_and_stats(pairs, sizes, tables)
    return bref.build(lifted, tables[3], r), stats


def stats_arrays(stats):
    """The statistics as the uint64 arrays the binding returns."""
    decay, cis, trans, unlifted = stats
    return (np.asarray(decay, np.uint64), np.asarray(cis, np.uint64), np.asarray(trans, np.uint64), np.asarray([unlifted], np.uint64))


def order_file_text(chromosomes, names):
    """An order file as Part 2 writes it."""
    out = []
    for c, chrom in enumerate(chromosomes, 1):
        out.append("### Chromosome grouping %d ###\n" % c)
        out += ["%s\t%s\n" % (names[s], o) for s, o in chrom]
    return "".join(out)
