"""NumPy restatement of DESIGN.md 9l - a raw contact map counted from HiC-Pro's valid pairs - for the tests of buildMap:
the text is parsed in plain Python, the cells are counted with ``np.add.at`` on the definition, and the upper triangle is
mirrored.  Nothing here calls the library."""
import re

import numpy as np

R = 1000                                                    # bin size of the hand-made cases
_INT = re.compile(rb"^ *[+-]?[0-9]+ *$")


class Malformed(ValueError):
    def __init__(self, offset):
        ValueError.__init__(self, "malformed valid-pair line at byte %d" % offset)
        self.offset = offset


def first_bins(sizes, r):
    """(first_bin per scaffold, m): a scaffold of length L has ceil(L / r) bins."""
    per = [-(-int(s) // int(r)) for s in sizes]
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64)[:-1], int(sum(per))


def bed_rows(names, sizes, r):
    """(name, start, stop, ID) of every bin of the grid at bin size r."""
    rows = []
    for name, size in zip(names, sizes):
        for k in range(-(-int(size) // r)):
            rows.append((name, k * r, min((k + 1) * r, int(size)), len(rows) + 1))
    return rows


def parse_text(data, names, sizes):
    """The kept pairs of the file's bytes, in file order, the statistics (lines, used, unknown_scaffold, out_of_range) and
    per kept pair the offset of the line after it.  Malformed: fewer than six columns or a non-integer position."""
    index = {}
    for k, name in enumerate(names):
        index.setdefault(name.encode("utf-8"), k)
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    kept, after = [], []
    n_lines = unknown = out_of_range = 0
    offset = 0
    for raw in lines:
        cols = raw.rstrip(b"\r").split(b"\t")
        if len(cols) < 6 or not _INT.match(cols[2]) or not _INT.match(cols[5]):
            raise Malformed(offset)
        offset = min(offset + len(raw) + 1, len(data))
        n_lines += 1
        a, b = index.get(cols[1], -1), index.get(cols[4], -1)
        p1, p2 = int(cols[2]), int(cols[5])
        if a < 0 or b < 0:
            unknown += 1
        elif p1 < 1 or p1 > sizes[a] or p2 < 1 or p2 > sizes[b]:
            out_of_range += 1
        else:
            kept.append((a, p1, b, p2))
            after.append(offset)
    arr = np.asarray(kept, dtype=np.int64).reshape(-1, 4)
    return ((arr[:, 0].astype(np.int32), arr[:, 1].copy(), arr[:, 2].astype(np.int32), arr[:, 3].copy()),
            (n_lines, len(kept), unknown, out_of_range), after)


def build(pairs, sizes, r):
    """The dense map of DESIGN.md 9l from (scaffold a, position a, scaffold b, position b) arrays."""
    sa, pa, sb, pb = (np.asarray(x, dtype=np.int64) for x in pairs)
    first, m = first_bins(sizes, r)
    i = first[sa] + (pa - 1) // r
    j = first[sb] + (pb - 1) // r
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    upper = np.zeros((m, m), dtype=np.uint64)
    np.add.at(upper, (lo, hi), 1)
    assert not np.tril(upper, -1).any()
    dense = upper.astype(np.float64)
    return dense + np.triu(dense, 1).T


# ---- hand-made inputs ------------------------------------------------------------------------------------------------
def odd_scaffolds(r=R):
    """40 scaffolds with the sizes 1, r - 1, r, r + 1, 3 r + 7 in turn and three of 70 r: 277 bins at r."""
    small = [1, r - 1, r, r + 1, 3 * r + 7]
    sizes = [small[k % 5] for k in range(40)]
    for k in (3, 17, 38):
        sizes[k] = 70 * r
    names = ["scaffold_%d" % (k + 1) for k in range(40)]
    return names, np.asarray(sizes, dtype=np.int64)


def edge_pairs(names, sizes, n, seed, r=R):
    """n pairs on the scaffolds: random ones, mixed with both mate orders of one pair, both ends in one bin, and the
    positions 1, k r, k r + 1 and L."""
    rng = np.random.default_rng(seed)
    S = len(names)
    sa, sb = rng.integers(0, S, n), rng.integers(0, S, n)
    pa = 1 + np.floor(rng.random(n) * sizes[sa]).astype(np.int64)
    pb = 1 + np.floor(rng.random(n) * sizes[sb]).astype(np.int64)
    kind = rng.integers(0, 8, n)
    same = kind == 0                                         # both ends in one bin
    sb[same] = sa[same]
    pb[same] = np.minimum(((pa[same] - 1) // r) * r + 1 + rng.integers(0, r, same.sum()), sizes[sa[same]])
    pa[kind == 1] = 1
    pb[kind == 2] = sizes[sb[kind == 2]]
    edge = kind == 3                                         # k r and k r + 1, where the scaffold is long enough
    k = rng.integers(1, 70, n)
    at = np.minimum(k * r, sizes[sa])
    pa[edge] = at[edge]
    edge1 = kind == 4
    pa[edge1] = np.minimum(k * r + 1, sizes[sa])[edge1]
    mirror = np.flatnonzero(kind == 5)                       # the pair before it, mates swapped
    mirror = mirror[mirror > 0]
    sa[mirror], pa[mirror], sb[mirror], pb[mirror] = sb[mirror - 1], pb[mirror - 1], sa[mirror - 1], pa[mirror - 1]
    return sa.astype(np.int32), pa, sb.astype(np.int32), pb


def odd_file_bytes(names, sizes, n_lines, seed):
    """An allValidPairs file of n_lines lines with: CRLF lines, 6- and 12-column lines, names of no scaffold in either
    column, the positions 0, 1, size and size + 1, blanks around a position, and no final newline."""
    rng = np.random.default_rng(seed)
    sa, pa, sb, pb = edge_pairs(names, sizes, n_lines, seed + 1)
    out = []
    for q in range(n_lines):
        a, b = names[sa[q]], names[sb[q]]
        x, y = int(pa[q]), int(pb[q])
        what = int(rng.integers(0, 24))
        if what == 0:
            a = "unplaced_7"
        elif what == 1:
            b = "scaffold_"                                    # a prefix of every name
        elif what == 2:
            x = 0
        elif what == 3:
            y = int(sizes[sb[q]]) + 1
        elif what == 4:
            x, y = 1, int(sizes[sb[q]])
        elif what == 5:
            x = int(sizes[sa[q]])
        xs = " %d " % x if what == 6 else "%d" % x
        line = "read%d\t%s\t%s\t+\t%s\t%d" % (q, a, xs, b, y)
        if what % 3:
            line += "\t-\t300\tf1\tf2\t42\t42"
        out.append(line + ("\r\n" if what % 4 == 1 else "\n"))
    text = "".join(out)
    return text[:-1].encode("ascii") if text.endswith("\n") and not text.endswith("\r\n") else text[:-2].encode("ascii")
