"""NumPy restatement of DESIGN.md 9n - the spanning depth of an assembly from read pairs - for the tests of supportSpans:
the cell numbering, the marks by ``np.add.at``, ``np.cumsum`` twice, the competing slots, the ratios and the first-minimum
picks; a second, brute-force depth counted from the definition; and a small generator of an assembly with a planted
misjoin.  Nothing here calls the library or the package."""
import numpy as np

MAX_FLANK = 4096
COUNTERS = ("marked", "one_cell", "beyond_max_span", "trans", "unlifted")


# ---- cells ---------------------------------------------------------------------------------------------------------------
def number_cells(sizes, tables, step):
    """(cell_first int64[S], seq_first int64[n_seq + 1], n_cells): a placed scaffold of size L > 0 has ceil(L / step)
    cells; sequences ascending, inside a sequence by offset; -1 for a dropped or empty scaffold."""
    seq, off, _rev, seq_sizes = tables
    cell_first = np.full(len(sizes), -1, np.int64)
    seq_first = [0]
    n = 0
    for q in range(len(seq_sizes)):
        members = [s for s in range(len(sizes)) if seq[s] == q and sizes[s] > 0]
        for s in sorted(members, key=lambda s: (int(off[s]), s)):
            cell_first[s] = n
            n += -(-int(sizes[s]) // int(step))
        seq_first.append(n)
    return cell_first, np.asarray(seq_first, np.int64), n


def lift(pairs, sizes, tables):
    """(sequence a, lifted a, sequence b, lifted b) as int64 arrays; sequence -1 (position 0) on a dropped scaffold."""
    seq, off, rev, _seq_sizes = tables
    sizes = np.asarray(sizes, np.int64)
    out = []
    for s, p in ((pairs[0], pairs[1]), (pairs[2], pairs[3])):
        s, p = np.asarray(s, np.int64), np.asarray(p, np.int64)
        q = seq[s].astype(np.int64)
        where = np.where(rev[s] != 0, sizes[s] - p + 1, p)
        out += [q, np.where(q >= 0, off[s] + where, 0)]
    return tuple(out)


def cells(pairs, sizes, tables, cell_first, step):
    """The global cell of both ends (meaningless where the scaffold is dropped)."""
    _seq, _off, rev, _seq_sizes = tables
    sizes = np.asarray(sizes, np.int64)
    out = []
    for s, p in ((pairs[0], pairs[1]), (pairs[2], pairs[3])):
        s, p = np.asarray(s, np.int64), np.asarray(p, np.int64)
        out.append(cell_first[s] + np.where(rev[s] != 0, sizes[s] - p, p - 1) // int(step))
    return out


def classify(pairs, sizes, tables, cell_first, step, max_span):
    """(kind per pair as an index into COUNTERS, lower cell, upper cell)."""
    qa, xa, qb, xb = lift(pairs, sizes, tables)
    ca, cb = cells(pairs, sizes, tables, cell_first, step)
    kind = np.zeros(len(qa), np.int64)
    far = np.abs(xa - xb) > max_span if max_span > 0 else np.zeros(len(qa), bool)
    kind[ca == cb] = 1
    kind[far] = 2
    kind[qa != qb] = 3
    kind[(qa < 0) | (qb < 0)] = 4
    return kind, np.minimum(ca, cb), np.maximum(ca, cb)


def depth(pairs, sizes, tables, step, max_span=0):
    """(D uint64[n_cells], counters uint64[5], marks uint64[n_cells]) by the marks and one prefix sum."""
    cell_first, _seq_first, n = number_cells(sizes, tables, step)
    kind, lo, hi = classify(pairs, sizes, tables, cell_first, step, max_span)
    marks = np.zeros(n, np.uint64)
    np.add.at(marks, lo[kind == 0], np.uint64(1))
    np.add.at(marks, hi[kind == 0], np.uint64(2 ** 64 - 1))              # -1 in two's complement
    with np.errstate(over="ignore"):
        D = np.cumsum(marks, dtype=np.uint64)
    return D, np.bincount(kind, minlength=5).astype(np.uint64), marks


def brute_depth(pairs, sizes, tables, step, max_span=0):
    """D straight from the definition: for every slot, the counted cis pairs with cell(a) <= c < cell(b)."""
    cell_first, _seq_first, n = number_cells(sizes, tables, step)
    qa, xa, qb, xb = lift(pairs, sizes, tables)
    ca, cb = cells(pairs, sizes, tables, cell_first, step)
    D = np.zeros(n, np.uint64)
    for k in range(len(qa)):
        if qa[k] < 0 or qb[k] < 0 or qa[k] != qb[k]:
            continue
        if max_span > 0 and abs(int(xa[k]) - int(xb[k])) > max_span:
            continue
        lo, hi = min(int(ca[k]), int(cb[k])), max(int(ca[k]), int(cb[k]))
        for c in range(n):
            if lo <= c < hi:
                D[c] += np.uint64(1)
    return D


# ---- flanks, ratios, picks ---------------------------------------------------------------------------------------------------
def flanks(D, flank, q0, q1):
    """(competes bool, Lsum, Rsum) of every slot c of the sequence with the cells [q0, q1), as arrays over q0 .. q1 - 1."""
    F, m = int(flank), int(q1 - q0)
    assert 1 <= F <= MAX_FLANK
    with np.errstate(over="ignore"):
        S = np.concatenate([[0], np.cumsum(np.asarray(D[q0:q1], np.uint64), dtype=np.uint64)]).astype(np.uint64)   # S[k] = d[0] + .. + d[k-1]
    comp, ls, rs = np.zeros(m, bool), np.zeros(m, np.int64), np.zeros(m, np.int64)
    c = np.arange(F, m - 1 - F)                                          # c - F >= 0 and c + F <= m - 2
    if len(c):
        ls[c] = (S[c] - S[c - F]).astype(np.int64)
        rs[c] = (S[c + F + 1] - S[c + 1]).astype(np.int64)
        comp[c] = np.minimum(ls[c], rs[c]) > 0
    return comp, ls, rs


def ratio(D_c, flank, lsum, rsum):
    """The ratio of a competing slot: one IEEE division of two integers below 2^53."""
    num, den = int(D_c) * int(flank), min(int(lsum), int(rsum))
    assert 0 < den < 2 ** 53 and num < 2 ** 53
    return float(num) / float(den)


def picks(D, flank, recs):
    """int64[n_rec, 4] = (slot, D, Lsum, Rsum): per record (lo, hi, q0, q1) the competing slot of lowest ratio, the first
    among equal ratios; (-1, 0, 0, 0) when nothing competes."""
    recs = np.asarray(recs, np.int64).reshape(-1, 4).tolist()
    out = np.zeros((len(recs), 4), np.int64)
    of_sequence = {}
    for r, (lo, hi, q0, q1) in enumerate(recs):
        assert 0 <= q0 <= lo <= hi < q1 <= len(D)
        if (q0, q1) not in of_sequence:
            of_sequence[(q0, q1)] = flanks(D, flank, q0, q1)
        comp, ls, rs = of_sequence[(q0, q1)]
        cand = [c for c in range(lo, hi + 1) if comp[c - q0]]
        if not cand:
            out[r] = (-1, 0, 0, 0)
            continue
        ratios = np.array([ratio(D[c], flank, ls[c - q0], rs[c - q0]) for c in cand])
        c = cand[int(np.argmin(ratios))]                                  # argmin takes the first minimum
        out[r] = (c, int(D[c]), ls[c - q0], rs[c - q0])
    return out


def pick_ratio(pick, flank):
    return None if pick[0] < 0 else ratio(pick[1], flank, pick[2], pick[3])


# ---- the records a report asks for -------------------------------------------------------------------------------------------
def components(sizes, tables):
    """Per sequence the placed scaffolds of size > 0 in sequence order."""
    seq, off, _rev, seq_sizes = tables
    return [sorted([s for s in range(len(sizes)) if seq[s] == q and sizes[s] > 0], key=lambda s: (int(off[s]), s))
            for q in range(len(seq_sizes))]


def report_records(sizes, tables, step):
    """(scaffold records {scaffold: (lo, hi, q0, q1)} over its interior boundaries - none for a scaffold of one cell -,
    junction records {(left, right): (c, c, q0, q1)} with c the last cell of the left scaffold)."""
    cell_first, seq_first, _n = number_cells(sizes, tables, step)
    scaf, junc = {}, {}
    for q, comps in enumerate(components(sizes, tables)):
        q0, q1 = int(seq_first[q]), int(seq_first[q + 1])
        for k, s in enumerate(comps):
            n = -(-int(sizes[s]) // int(step))
            if n >= 2:
                scaf[s] = (int(cell_first[s]), int(cell_first[s]) + n - 2, q0, q1)
            if k + 1 < len(comps):
                junc[(s, comps[k + 1])] = (int(cell_first[s]) + n - 1, int(cell_first[s]) + n - 1, q0, q1)
    return scaf, junc


# ---- an assembly with a planted misjoin ----------------------------------------------------------------------------------------
PLANTED_STEP, PLANTED_FLANK, PLANTED_MIN_RATIO = 1000, 8, 0.2


def planted(seed=11, n_cis=60000, n_trans=800):
    """A true genome of three chromosomes and one small contig, cut into scaffolds; cis pairs with a heavy-tailed
    (log-uniform) distance plus uniform trans noise.  Two errors are planted in the assembly: scaffold ``glued`` is the end of
    chromosome 1 with the end of chromosome 2 glued on (the joint lies after its base ``glue_at``), and the last scaffold of
    chromosome 3 is placed after the last one of chromosome 2 (``false_junction``).  Returns a dict with names, sizes,
    chroms [[(scaffold, "+" / "-"), ...], ...] (the contig stays unplaced), pairs and the three truths."""
    rng = np.random.default_rng(seed)
    chrom_len = [120000, 90000, 100000, 12000]
    piece = 15000
    # pieces of the true genome: (chromosome, start, length, scaffold, offset in the scaffold, scaffold reversed to the truth)
    pieces, names, sizes, chroms = [], [], [], [[], [], []]
    cuts = {0: [18000, 25000, 21000, 16000, 25000], 1: [22000, 17000, 20000, 16000], 2: [19000, 24000, 17000, 25000]}

    def scaffold(size):
        names.append("scaf_%d" % (len(names) + 1))
        sizes.append(size)
        return len(names) - 1

    tail = {}
    for c in range(3):
        at = 0
        for L in cuts[c]:
            s = scaffold(L)
            flipped = bool(rng.integers(0, 2))
            pieces.append((c, at, L, s, 0, flipped))
            chroms[c].append((s, "-" if flipped else "+"))
            at += L
        tail[c] = at
        assert chrom_len[c] - at == piece
    glued = scaffold(2 * piece)                                          # the end of chromosome 1, then the end of chromosome 2
    pieces.append((0, tail[0], piece, glued, 0, False))
    pieces.append((1, tail[1], piece, glued, piece, False))
    chroms[0].append((glued, "+"))
    last3 = scaffold(piece)                                              # the end of chromosome 3, placed after chromosome 2
    pieces.append((2, tail[2], piece, last3, 0, False))
    false_junction = (chroms[1][-1][0], last3)
    chroms[1].append((last3, "+"))
    contig = scaffold(chrom_len[3])
    pieces.append((3, 0, chrom_len[3], contig, 0, False))
    sizes = np.asarray(sizes, np.int64)

    g_start = np.concatenate([[0], np.cumsum(chrom_len)])               # the chromosomes laid end to end: global coordinates
    table = sorted((int(g_start[c]) + start, L, s, o, f) for c, start, L, s, o, f in pieces)
    p_start = np.array([t[0] for t in table])

    def place(x):                                                        # 0-based global coordinate -> (scaffold, 1-based position)
        k = np.searchsorted(p_start, x, side="right") - 1
        s = np.array([t[2] for t in table])[k]
        o = np.array([t[3] for t in table])[k]
        f = np.array([t[4] for t in table])[k]
        inside = o + (x - p_start[k])
        return s.astype(np.int32), np.where(f, sizes[s] - inside, inside + 1).astype(np.int64)

    weights = np.asarray(chrom_len, float) / sum(chrom_len)
    c = rng.choice(4, n_cis, p=weights)
    a = np.floor(rng.random(n_cis) * np.asarray(chrom_len)[c]).astype(np.int64)
    d = np.exp(rng.uniform(np.log(100.0), np.log(50000.0), n_cis)).astype(np.int64) * rng.choice([-1, 1], n_cis)
    b = a + d
    ok = (b >= 0) & (b < np.asarray(chrom_len)[c])
    xa, xb = g_start[c][ok] + a[ok], g_start[c][ok] + b[ok]
    total = int(g_start[-1])
    xa = np.concatenate([xa, rng.integers(0, total, n_trans)])
    xb = np.concatenate([xb, rng.integers(0, total, n_trans)])
    mix = rng.permutation(len(xa))
    sa, pa = place(xa[mix])
    sb, pb = place(xb[mix])
    return {"names": names, "sizes": sizes, "chroms": chroms, "pairs": (sa, pa, sb, pb), "glued": glued, "glue_at": piece,
            "false_junction": false_junction, "contig": contig}


def pair_file_bytes(names, pairs):
    """The pairs as an allValidPairs file."""
    sa, pa, sb, pb = (np.asarray(x).tolist() for x in pairs)
    return "".join("r%d\t%s\t%d\t+\t%s\t%d\t-\n" % (k, names[sa[k]], pa[k], names[sb[k]], pb[k]) for k in range(len(sa))).encode("ascii")
