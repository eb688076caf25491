"""TEST INFRASTRUCTURE: the junction-support report restated with NumPy.  Nothing here calls the product's
junction code: a side is an explicit index array, a sum is ``(M[np.ix_(A, B)] * W).sum()`` with ``W[a][b] = 1.0 /
(a + b + 1)``, the norm is counted with ``np.bincount``, the report text is formatted by a restatement of the file format,
and joins and cuts are applied to plain lists - the joins Kruskal-fashion, the largest J first, so that the join which
would close a cycle is its smallest - not by walking the ends as the product does."""
import numpy as np

END = ("head", "tail")


def chromosome_sides(chrom_rows, arrangement, where):
    """[(scaffold, matrix indices in reading order)] of one chromosome: ``chrom_rows`` the group file's [bin ID,
    scaffold] rows, ``arrangement`` its [(scaffold, '+'/'-')] of the order file, ``where`` {bin ID: matrix index}."""
    bins_of = {}
    for bin_id, name in chrom_rows:
        bins_of.setdefault(name, []).append(bin_id)
    out = []
    for name, orient in arrangement:
        idx = [where[b] for b in sorted(bins_of[name])]
        out.append((name, idx[::-1] if orient == "-" else idx))
    return out


def weights(lenA, lenB):
    return 1.0 / (np.arange(lenA)[:, None] + np.arange(lenB)[None, :] + 1)


def norm(lenA, lenB):
    """cnt(d) * (1.0 / d) added for d = 1, 2, ... in that order, cnt counted from the pairs themselves."""
    cnt = np.bincount((np.arange(lenA)[:, None] + np.arange(lenB)[None, :] + 1).ravel())
    acc = 0.0
    for d in range(1, len(cnt)):
        acc += float(cnt[d]) * (1.0 / d)
    return acc


def side_sum(M, A, B):
    return float((M[np.ix_(A, B)] * weights(len(A), len(B))).sum())


def record_sums(M, bins, rec):
    """hicmi_junction_sums restated: bins and six-valued records as the export takes them."""
    bins = np.asarray(bins)
    out = []
    for sa, ta, la, sb, tb, lb in np.asarray(rec).tolist():
        out.append(side_sum(M, bins[sa + ta * np.arange(la)], bins[sb + tb * np.arange(lb)]))
    return np.array(out)


def analyse(M, chromosomes, window=16, min_rel=0.25):
    """``chromosomes``: per chromosome chromosome_sides' list.  Returns a dict: ref, junctions (per chromosome a list of
    dicts), ends (2G dicts), table, joins [((c, end), (c2, end2), J)] with the lower end first, weak [(c, k)], sums (the
    raw sums: internal junctions chromosome by chromosome, then end pairs e < f on different chromosomes)."""
    take = (lambda v: v[:window]) if window else (lambda v: v)
    G = len(chromosomes)
    flat = [[i for _n, idx in chrom for i in idx] for chrom in chromosomes]
    sums, junctions = [], []
    for chrom, order in zip(chromosomes, flat):
        rows, at = [], 0
        for k in range(len(chrom) - 1):
            at += len(chrom[k][1])
            A, B = take(order[:at][::-1]), take(order[at:])
            s = side_sum(M, A, B)
            sums.append(s)
            rows.append({"left": chrom[k][0], "right": chrom[k + 1][0], "bins_left": len(A), "bins_right": len(B),
                         "J": s / norm(len(A), len(B))})
        junctions.append(rows)
    all_J = [r["J"] for rows in junctions for r in rows]
    ref = float(np.median(all_J)) if all_J else None
    if ref is not None and ref == 0:
        ref = None
    weak = []
    for c, rows in enumerate(junctions):
        for k, r in enumerate(rows):
            r["rel"] = None if ref is None else r["J"] / ref
            r["verdict"] = "NA" if ref is None else ("held" if r["rel"] >= min_rel else "weak")
            if r["verdict"] == "weak":
                weak.append((c, k))
    sides = []
    for order in flat:
        sides.append(take(order))
        sides.append(take(order[::-1]))
    table = np.full((2 * G, 2 * G), np.nan)
    for e in range(2 * G):
        for f in range(e + 1, 2 * G):
            if e // 2 != f // 2:
                s = side_sum(M, sides[e], sides[f])
                sums.append(s)
                table[e, f] = table[f, e] = s / norm(len(sides[e]), len(sides[f]))

    def arg_first_max(e, banned):
        cand = [f for f in range(2 * G) if f // 2 not in banned]
        if not cand:
            return None
        vals = [table[e, f] for f in cand]
        return cand[int(np.argmax(vals))]                    # np.argmax: the first of equal maxima
    best = [arg_first_max(e, {e // 2}) for e in range(2 * G)]
    ends, joins = [], []
    for e in range(2 * G):
        f = best[e]
        row = {"chromosome": e // 2, "end": END[e % 2], "scaffold": chromosomes[e // 2][-1 if e % 2 else 0][0],
               "bins": len(sides[e]), "best": f}
        if f is None:
            row.update(J=None, rel=None, mutual=None, second=None, second_J=None, verdict="NA")
        else:
            g = arg_first_max(e, {e // 2, f // 2})
            row.update(J=float(table[e, f]), mutual=best[f] == e, second=g,
                       second_J=None if g is None else float(table[e, g]))
            row["rel"] = None if ref is None else row["J"] / ref
            row["verdict"] = "NA" if ref is None else ("joinable" if row["mutual"] and row["rel"] >= min_rel else "free")
            if row["verdict"] == "joinable" and e < f:
                joins.append(((e // 2, e % 2), (f // 2, f % 2), row["J"]))
        ends.append(row)
    return {"ref": ref, "window": window, "min_rel": min_rel, "junctions": junctions, "ends": ends, "table": table,
            "joins": joins, "weak": weak, "sums": np.array(sums), "names": [[n for n, _i in ch] for ch in chromosomes]}


def _txt(v):
    return "NA" if v is None else (repr(v) if isinstance(v, float) else str(v))


def report_text(res):
    out = ["### reference %s window %d minRel %s\n" % (_txt(res["ref"]), res["window"], repr(float(res["min_rel"])))]
    for c, rows in enumerate(res["junctions"]):
        out.append("### Chromosome grouping %d ###\n" % (c + 1))
        for r in rows:
            out.append("\t".join([r["left"], r["right"], str(r["bins_left"]), str(r["bins_right"]), repr(r["J"]),
                                  _txt(r["rel"]), r["verdict"]]) + "\n")
    out.append("### Chromosome ends ###\n")
    for r in res["ends"]:
        f, g = r["best"], r["second"]
        out.append("\t".join([str(r["chromosome"] + 1), r["end"], r["scaffold"], str(r["bins"]),
                              "NA" if f is None else str(f // 2 + 1), "NA" if f is None else END[f % 2], _txt(r["J"]),
                              _txt(r["rel"]), "NA" if r["mutual"] is None else ("yes" if r["mutual"] else "no"),
                              "NA" if g is None else str(g // 2 + 1), _txt(r["second_J"]), r["verdict"]]) + "\n")
    return "".join(out)


def _turned(strand):
    return [(c, not rev) for c, rev in strand[::-1]]


def join_plain(arrangements, joins):
    """``arrangements``: per chromosome [(scaffold, '+'/'-')]; ``joins``: [((c, end), (c2, end2), J)], end 0 head, 1 tail.
    Returns (joined arrangements, members per joined chromosome [(c, reversed)], dropped joins in listing order)."""
    strands = [[(c, False)] for c in range(len(arrangements))]
    dropped = []

    def open_ends(strand):                                    # (left end, right end) of a strand
        (c0, r0), (c1, r1) = strand[0], strand[-1]
        return (c0, 1 if r0 else 0), (c1, 0 if r1 else 1)
    order = sorted(range(len(joins)), key=lambda i: (-joins[i][2], -i))
    for i in order:
        e, f, _J = joins[i]
        se = next(s for s in strands if any(c == e[0] for c, _r in s))
        sf = next(s for s in strands if any(c == f[0] for c, _r in s))
        if se is sf:
            dropped.append(i)
            continue
        if open_ends(se)[1] != e:
            se2 = _turned(se)
        else:
            se2 = se
        sf2 = sf if open_ends(sf)[0] == f else _turned(sf)
        assert open_ends(se2)[1] == e and open_ends(sf2)[0] == f, "an end joined twice"
        strands = [s for s in strands if s is not se and s is not sf] + [se2 + sf2]
    final = []
    for s in strands:
        low = min(c for c, _r in s)
        if dict(s)[low]:
            s = _turned(s)
        final.append((low, s))
    final.sort()
    out = []
    for _low, s in final:
        chrom = []
        for c, rev in s:
            a = arrangements[c]
            chrom.extend([(n, "+" if o == "-" else "-") for n, o in a[::-1]] if rev else a)
        out.append(chrom)
    return out, [s for _low, s in final], [joins[i] for i in sorted(dropped)]


def cut_plain(arrangements, weak):
    out = []
    for c, a in enumerate(arrangements):
        marks = sorted(k + 1 for cc, k in weak if cc == c)
        for lo, hi in zip([0] + marks, marks + [len(a)]):
            out.append(a[lo:hi])
    return out


def order_text(arrangements):
    return "".join("### Chromosome grouping %d ###\n" % (k + 1) + "".join(n + "\t" + o + "\n" for n, o in a)
                   for k, a in enumerate(arrangements))


class NumpyJunctionContext:
    """Answers Context.junction_sums with record_sums: lets the CPU suite run the product's host flow."""

    def __init__(self, M):
        self.mat = np.asarray(M, dtype=np.float64)
        self.n = len(self.mat)

    def junction_sums(self, bins, rec):
        return record_sums(self.mat, bins, rec)

    def close(self):
        pass
