// span.h - spanning depth: the cells a placed scaffold is cut into, the cell of a read end, what a pair
// marks, and which slots compete for a pick.  Like liftmap.h it is plain integer arithmetic without a GPU dependency:
// the kernels of k_spans.hip and api.hip include it, and so does a stand-alone host program built with the sanitizers
// (tests/span_host_check.cpp).
#pragma once
#include "liftmap.h"

namespace hicmi {

constexpr int64_t SPAN_MAX_CELLS = (int64_t)1 << 27;
constexpr int64_t SPAN_MAX_FLANK = 4096;

// what a pair is to the depth; the value is the index of its counter
enum SpanKind { SPAN_MARKED = 0, SPAN_ONE_CELL = 1, SPAN_TOO_FAR = 2, SPAN_TRANS = 3, SPAN_UNLIFTED = 4, SPAN_COUNTERS = 5,
                SPAN_NOWHERE = -1 };

// The cells of a build: cell_first per scaffold (-1: dropped or empty; device memory in a kernel), the cell size and
// the longest lifted distance that counts (0: no limit).
struct SpanGrid {
    const int64_t* cell_first = nullptr;
    int64_t step = 1, max_span = 0, n_cells = 0;
};

// ceil(len / step) for len >= 0, without the sum len + step - 1
LIFT_HD int64_t span_cells_of(int64_t len, int64_t step) { return len / step + (len % step != 0); }

// Local cell of the 1-based position p on a scaffold of length len: cells are cut from the scaffold's left end as it
// lies in its sequence, which is its base len when it is reversed.
LIFT_HD int64_t span_local_cell(int64_t len, int64_t p, bool rev, int64_t step)
{
    const int64_t x = rev ? len - p : p - 1;
    if (((uint64_t)x | (uint64_t)step) >> 32) return x / step;
    return (int64_t)((uint32_t)x / (uint32_t)step);                     // the usual case: 32-bit division
}

// What the pair (sa, pa, sb, pb) is, and for SPAN_MARKED its cells ordered, *lo_out < *hi_out: it adds +1 at slot lo and
// -1 at slot hi.  SPAN_NOWHERE: an end outside the tables or its scaffold (the host refuses those before a chunk is
// uploaded).  The distance limit is looked at before the cells, so a pair beyond it counts as SPAN_TOO_FAR even when
// both ends share a cell.
LIFT_HD int span_classify(const LiftTables& L, const SpanGrid& G, int32_t sa, int64_t pa, int32_t sb, int64_t pb, int64_t* lo_out,
                          int64_t* hi_out)
{
    int32_t qa, qb;
    int64_t ya = 0, yb = 0;
    const bool ok_a = lift_end(L, sa, pa, &qa, &ya), ok_b = lift_end(L, sb, pb, &qb, &yb);
    if (!ok_a || !ok_b) return qa >= -1 && qb >= -1 ? SPAN_UNLIFTED : SPAN_NOWHERE;
    if (qa != qb) return SPAN_TRANS;
    const uint64_t d = ya < yb ? (uint64_t)(yb - ya) : (uint64_t)(ya - yb);
    if (G.max_span > 0 && d > (uint64_t)G.max_span) return SPAN_TOO_FAR;
    const int64_t fa = G.cell_first[sa], fb = G.cell_first[sb];
    if (fa < 0 || fb < 0) return SPAN_NOWHERE;                          // an end on an empty scaffold: there is none
    const int64_t ca = fa + span_local_cell(L.scaf_size[sa], pa, L.rev[sa] != 0, G.step);
    const int64_t cb = fb + span_local_cell(L.scaf_size[sb], pb, L.rev[sb] != 0, G.step);
    if (ca < 0 || cb < 0 || ca >= G.n_cells || cb >= G.n_cells) return SPAN_NOWHERE;
    if (ca == cb) return SPAN_ONE_CELL;
    *lo_out = ca < cb ? ca : cb;
    *hi_out = ca < cb ? cb : ca;
    return SPAN_MARKED;
}

// Does slot c of the sequence with the cells [q0, q1) compete at a flank of F slots?  S is the inclusive prefix sum of
// the depth D over all cells (unsigned: differences are exact although S itself may wrap).  The flanks are
//   Lsum = D[c - F] + .. + D[c - 1],   Rsum = D[c + 1] + .. + D[c + F]
// and must lie inside the sequence without its last slot, the terminator; the smaller one must not be 0.
LIFT_HD bool span_competes(const unsigned long long* S, int64_t c, int64_t F, int64_t q0, int64_t q1, unsigned long long* lsum_out,
                           unsigned long long* rsum_out)
{
    if (c - F < q0 || c + F > q1 - 2) return false;
    const unsigned long long before = c - F > 0 ? S[c - F - 1] : 0ull;
    const unsigned long long lsum = (c > 0 ? S[c - 1] : 0ull) - before, rsum = S[c + F] - S[c];
    *lsum_out = lsum; *rsum_out = rsum;
    return (lsum < rsum ? lsum : rsum) > 0;
}

// The ratio of a competing slot: one IEEE division of two integers below 2^53, both converted exactly
LIFT_HD double span_ratio(unsigned long long depth, int64_t F, unsigned long long lsum, unsigned long long rsum)
{
    return (double)(depth * (unsigned long long)F) / (double)(lsum < rsum ? lsum : rsum);
}

// The pick of the record (lo, hi, q0, q1): the competing slot of [lo, hi] with the lowest ratio, the lowest slot among
// equal ratios; out4 = slot, D, Lsum, Rsum, or -1, 0, 0, 0 when nothing competes.  The host's form of k_span_pick.
inline void span_pick(const unsigned long long* D, const unsigned long long* S, int64_t F, int64_t lo, int64_t hi, int64_t q0,
                      int64_t q1, int64_t* out4)
{
    out4[0] = -1; out4[1] = out4[2] = out4[3] = 0;
    double best = 0.0;
    for (int64_t c = lo; c <= hi; c++) {
        unsigned long long ls, rs;
        if (!span_competes(S, c, F, q0, q1, &ls, &rs)) continue;
        const double ratio = span_ratio(D[c], F, ls, rs);
        if (out4[0] < 0 || ratio < best) { best = ratio; out4[0] = c; out4[1] = (int64_t)D[c]; out4[2] = (int64_t)ls; out4[3] = (int64_t)rs; }
    }
}

// The cell numbering of a build on the host, from tables that passed lift_check_tables: sequences ascending, inside a
// sequence the scaffolds by offset.  cell_first[n_scaf] (-1 for a dropped or empty scaffold), seq_first[n_seq + 1] (the
// cells of sequence q are [seq_first[q], seq_first[q + 1]): none when it holds no placed base).  Returns the number of
// cells, or -1 as soon as it passes SPAN_MAX_CELLS.
inline int64_t span_number_cells(const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                                 int64_t n_seq, int64_t step, int64_t* cell_first, int64_t* seq_first)
{
    std::vector<int64_t> placed;
    for (int64_t s = 0; s < n_scaf; s++) {
        cell_first[s] = -1;
        if (lift_seq[s] >= 0 && scaf_size[s] > 0) placed.push_back(s);
    }
    std::sort(placed.begin(), placed.end(), [&](int64_t a, int64_t b) {
        if (lift_seq[a] != lift_seq[b]) return lift_seq[a] < lift_seq[b];
        if (lift_off[a] != lift_off[b]) return lift_off[a] < lift_off[b];
        return a < b;
    });
    int64_t n = 0, q = 0;
    seq_first[0] = 0;
    for (const int64_t s : placed) {
        while (q < lift_seq[s]) seq_first[++q] = n;
        cell_first[s] = n;
        const int64_t cells = span_cells_of(scaf_size[s], step);
        if (cells > SPAN_MAX_CELLS - n) return -1;
        n += cells;
    }
    while (q < n_seq) seq_first[++q] = n;
    return n;
}

}  // namespace hicmi
