"""Group support restated in dense NumPy, independent of the package's implementation.

``group_sums`` fixes the summation order with ``numpy.cumsum`` (strictly left to right): the members of a group by
ascending row index in chunks of 64, every chunk from 0.0, the chunk sums left to right, a scaffold's bins left to right in
bin-list order.  A device result is compared with ``==``.

``records`` turns the two tables into one record per scaffold (assigned / best / second / ratio / verdict / runs), and
``report_text`` / ``rescued_text`` into the two files.  The readers below parse the HiC-Pro bed and a chromosomeGroupFile
on their own.
"""
import numpy as np

CHUNK = 64


def group_sums(M, grp, scaf, n_groups, n_scaffolds):
    """(binsum n x G, scafsum S x G).  binsum[i][g] = sum of M[j][i] over the rows j with grp[j] == g and
    scaf[j] != scaf[i]; scafsum[s][g] = sum of binsum[i][g] over the bins i of s."""
    M = np.asarray(M, dtype=np.float64)
    grp = np.asarray(grp)
    scaf = np.asarray(scaf)
    n = M.shape[0]
    binsum = np.zeros((n, n_groups))
    for g in range(n_groups):
        rows = np.flatnonzero(grp == g)                       # ascending
        chunk_sums = []
        for c0 in range(0, len(rows), CHUNK):
            r = rows[c0:c0 + CHUNK]
            vals = np.where(scaf[r][:, None] != scaf[None, :], M[r, :], 0.0)
            chunk_sums.append(np.cumsum(np.vstack([np.zeros((1, n)), vals]), axis=0)[-1])
        if chunk_sums:
            binsum[:, g] = np.cumsum(np.vstack(chunk_sums), axis=0)[-1]
    scafsum = np.zeros((n_scaffolds, n_groups))
    for s in range(n_scaffolds):
        bins = np.flatnonzero(scaf == s)                      # bin-list order
        if len(bins):
            scafsum[s] = np.cumsum(binsum[bins, :], axis=0)[-1]
    return binsum, scafsum


def read_bed(bed_file):
    """[(scaffold, bin ID)] in file order."""
    out = []
    with open(bed_file) as fh:
        for line in fh:
            cols = line.rstrip("\r\n").split("\t")
            out.append((cols[0], int(cols[3])))
    return out


def scaffold_bin_counts(bed):
    """{scaffold: bins in the bed}, in first-appearance order."""
    counts = {}
    for name, _bid in bed:
        counts[name] = counts.get(name, 0) + 1
    return counts


def read_group_file(path):
    """[(header line, [lines])] of a chromosomeGroupFile; every '#' line starts a group."""
    groups = []
    with open(path) as fh:
        for line in fh.read().splitlines():
            if line.startswith("#"):
                groups.append((line, []))
            else:
                groups[-1][1].append(line)
    return groups


def labels_of(groups, bin_ids):
    """grp[i] of every bin of ``bin_ids``: the index of the group whose lines name it, else -1."""
    where = {}
    for g, (_head, lines) in enumerate(groups):
        for ln in lines:
            where[int(ln.split("\t")[0])] = g
    return np.array([where.get(int(b), -1) for b in bin_ids], dtype=np.int64)


def _rle(labels):
    out, k = [], 0
    while k < len(labels):
        j = k
        while j < len(labels) and labels[j] == labels[k]:
            j += 1
        out.append("%s:%d" % (labels[k], j - k))
        k = j
    return ",".join(out) if out else "NA"


def records(M, bin_ids, bin_scaffolds, groups, bin_counts, min_ratio=3.0, live_is_all=False):
    """One record per scaffold of ``bin_counts`` (bed order).  ``M``: the map over the bins ``bin_ids`` (their scaffolds:
    ``bin_scaffolds``), zero rows compacted away or not.  ``live_is_all``: L_s = every bin of the scaffold in the map
    (the prototype's |s|) instead of the bins with a non-zero row sum."""
    M = np.asarray(M, dtype=np.float64)
    n, G = M.shape[0], len(groups)
    names = list(bin_counts)
    sid = {name: k for k, name in enumerate(names)}
    scaf = np.array([sid[s] for s in bin_scaffolds], dtype=np.int64)
    live = np.ones(n, dtype=bool) if live_is_all else M.sum(axis=1) != 0
    grp = labels_of(groups, bin_ids)
    grp[~(M.sum(axis=1) != 0)] = -1                           # a label on a zero row is ignored
    S = len(names)
    binsum, scafsum = group_sums(M, grp, scaf, G, S)
    m = np.array([int(np.count_nonzero(grp == g)) for g in range(G)])
    out = []
    for s, name in enumerate(names):
        bins = np.flatnonzero(scaf == s)
        own = np.array([int(np.count_nonzero(grp[bins] == g)) for g in range(G)])
        lb = bins[live[bins]]
        L = len(lb)
        pairs = L * (m - own)
        dens = np.array([scafsum[s][g] / pairs[g] if pairs[g] else 0.0 for g in range(G)])
        rec = {"scaffold": name, "bins": bin_counts[name], "live_bins": L, "density": dens.tolist(),
               "assigned": int(np.argmax(own)) if own.any() else None,
               "best": None, "best_density": None, "second": None, "second_density": None, "ratio": None,
               "live_ids": sorted(int(bin_ids[i]) for i in lb)}
        if L == 0 or not dens.any():
            rec["verdict"] = "no_contacts"
        else:
            best = int(np.argmax(dens))                       # the first of equals
            rec["best"], rec["best_density"] = best, float(dens[best])
            if G > 1:
                rest = dens.copy()
                rest[best] = -np.inf
                second = int(np.argmax(rest))
                rec["second"], rec["second_density"] = second, float(dens[second])
                rec["ratio"] = float(dens[best] / dens[second]) if dens[second] != 0.0 else float("inf")
            else:
                rec["ratio"] = float("inf")
            if rec["assigned"] is not None:
                rec["verdict"] = "supported" if best == rec["assigned"] else "contested"
            else:
                rec["verdict"] = "rescued" if rec["ratio"] >= min_ratio else "ambiguous"
        side = []
        for i in sorted(lb, key=lambda i: int(bin_ids[i])):
            denom = m - own
            v = np.array([binsum[i][g] / denom[g] if denom[g] else 0.0 for g in range(G)])
            side.append(str(int(np.argmax(v)) + 1) if v.any() else "-")
        rec["runs"] = _rle(side)
        out.append(rec)
    return out


def _text(v):
    return "NA" if v is None else (repr(v) if isinstance(v, float) else str(v))


def _group_number(g):
    return None if g is None else g + 1


HEADER = "#scaffold\tbins\tlive_bins\tassigned\tbest\tbest_density\tsecond\tsecond_density\tratio\tverdict\truns\n"


def report_text(recs):
    text = [HEADER]
    for r in recs:
        text.append("\t".join([r["scaffold"], str(r["bins"]), str(r["live_bins"]), _text(_group_number(r["assigned"])),
                               _text(_group_number(r["best"])), _text(r["best_density"]), _text(_group_number(r["second"])),
                               _text(r["second_density"]), _text(r["ratio"]), r["verdict"], r["runs"]]) + "\n")
    return "".join(text)


def rescued_text(recs, groups):
    text = []
    for g, (head, lines) in enumerate(groups):
        text.append(head + "\n")
        text.extend(ln + "\n" for ln in lines)
        for r in recs:
            if r["verdict"] == "rescued" and r["best"] == g:
                text.extend("%d\t%s\n" % (b, r["scaffold"]) for b in r["live_ids"])
    return "".join(text)


def verdict_counts(recs):
    out = {}
    for r in recs:
        out[r["verdict"]] = out.get(r["verdict"], 0) + 1
    return out


def case_inputs(bed, M_full, nan_ids=()):
    """(map, bin IDs, scaffolds of the bins) of a case as the loaders see it: bins with a NaN bias are not loaded."""
    keep = [k for k, (_s, b) in enumerate(bed) if b not in set(nan_ids)]
    M = np.ascontiguousarray(np.asarray(M_full)[np.ix_(keep, keep)])
    return M, [bed[k][1] for k in keep], [bed[k][0] for k in keep]


def withhold(groups, bin_counts, step=5):
    """The leave-out experiment's group file: every ``step``-th assigned scaffold, in bed (scaffold-id) order, loses its
    lines.  Returns (groups without them, {withheld scaffold: its original group})."""
    home = {}
    for g, (_h, lines) in enumerate(groups):
        for ln in lines:
            home.setdefault(ln.split("\t")[1], g)
    assigned = [s for s in bin_counts if s in home]
    gone = {s: home[s] for s in assigned[::step]}
    kept = [(h, [ln for ln in lines if ln.split("\t")[1] not in gone]) for h, lines in groups]
    return kept, gone
