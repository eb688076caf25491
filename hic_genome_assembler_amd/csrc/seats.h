// seats.h - seat support: every placed scaffold taken out of its ordering and re-placed from its read pairs.
// The blocks of counters the placed scaffolds own, the kind of a pair and the up to four counters it adds to.  Like ends.h
// and anchor.h it is plain integer arithmetic without a GPU dependency: the kernel of k_seats.hip and api.hip include it,
// and so does a stand-alone host program built with the sanitizers (tests/seats_host_check.cpp).
#pragma once
#include "anchor.h"

namespace hicmi {

constexpr int64_t SEATS_MAX_TABLE = (int64_t)1 << 27;     // counters of a table: the blocks of all placed scaffolds

// what a pair is to the table; the value is the index of its counter.  A pair is checked for NOWHERE, UNLIFTED and SAME
// in this order; what is left adds its two chromosome counters and is TRANS, or SEATED with a gap counter, or MIDDLE.
enum SeatsKind { SEATS_SEATED = 0, SEATS_MIDDLE = 1, SEATS_TRANS = 2, SEATS_SAME = 3, SEATS_UNLIFTED = 4, SEATS_COUNTERS = 5,
                 SEATS_NOWHERE = -1 };

// The blocks of a call (device memory in a kernel): first per scaffold (-1: dropped or empty), the rank per scaffold and
// seq_first[n_seq + 1] of ends_number_ranks at reach 1, and the window in bases.
struct SeatsGrid {
    const int64_t* first = nullptr;
    const int32_t* rank = nullptr;
    const int64_t* seq_first = nullptr;
    int64_t window = 1;
};

// What the pair (sa, pa, sb, pb) is, and the counters it adds 1 to: index_out[0 .. *n_out).  A pair between two placed
// scaffolds is evidence about the seat of both.  Chromosome counters: first[sa] + q_b and first[sb] + q_a.  Gap counters,
// inside one sequence q: first[c] + n_seq + k * 4 + half * 2 + zone for c = sa with the other end on sb and for c = sb
// with the other end on sa - k the local rank of the other scaffold in q, half the half of c its own end falls in
// (anchor_half, c's + coordinates), zone the end zone of the other end as it lies (ends_zone) - unless that zone is
// ENDS_MID.  The row k = k_c of c's own block is never indexed: sa != sb here.
LIFT_HD int seats_classify(const LiftTables& L, const SeatsGrid& G, int32_t sa, int64_t pa, int32_t sb, int64_t pb, int64_t* index_out,
                           int* n_out)
{
    *n_out = 0;
    int32_t qa, qb;
    int64_t ya = 0, yb = 0;
    const bool ok_a = lift_end(L, sa, pa, &qa, &ya), ok_b = lift_end(L, sb, pb, &qb, &yb);
    if ((!ok_a && qa != -1) || (!ok_b && qb != -1)) return SEATS_NOWHERE;
    if (!ok_a || !ok_b) return SEATS_UNLIFTED;
    if (sa == sb) return SEATS_SAME;
    const int64_t fa = G.first[sa], fb = G.first[sb];
    if (fa < 0 || fb < 0) return SEATS_NOWHERE;
    index_out[0] = fa + qb;
    index_out[1] = fb + qa;
    *n_out = 2;
    if (qa != qb) return SEATS_TRANS;
    const int64_t q0 = G.seq_first[qa], S = G.seq_first[qa + 1] - q0;
    const int64_t ka = (int64_t)G.rank[sa] - q0, kb = (int64_t)G.rank[sb] - q0;
    if (G.rank[sa] < 0 || G.rank[sb] < 0 || ka < 0 || ka >= S || kb < 0 || kb >= S) { *n_out = 0; return SEATS_NOWHERE; }
    int n = 2;
    const int zb = ends_zone(L.scaf_size[sb], pb, L.rev[sb] != 0, G.window);
    if (zb != ENDS_MID) index_out[n++] = fa + L.n_seq + kb * 4 + anchor_half(L.scaf_size[sa], pa) * 2 + zb;
    const int za = ends_zone(L.scaf_size[sa], pa, L.rev[sa] != 0, G.window);
    if (za != ENDS_MID) index_out[n++] = fb + L.n_seq + ka * 4 + anchor_half(L.scaf_size[sb], pb) * 2 + za;
    *n_out = n;
    return n > 2 ? SEATS_SEATED : SEATS_MIDDLE;
}

// The blocks of a call on the host, from tables that passed lift_check_tables and the rank and seq_first of
// ends_number_ranks at reach 1: the placed scaffolds with a base in index order, each with a block of
// n_seq + 4 x (placed scaffolds of its sequence) counters.  first[n_scaf] (-1 for a dropped or empty scaffold).  Returns
// the size of the table - 0: no scaffold is placed - or -1 as soon as it passes SEATS_MAX_TABLE.
inline int64_t seats_number_blocks(const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, int64_t n_seq, const int64_t* seq_first,
                                   int64_t* first)
{
    int64_t total = 0;
    for (int64_t s = 0; s < n_scaf; s++) {
        first[s] = -1;
        if (lift_seq[s] < 0 || scaf_size[s] <= 0) continue;
        // a sequence has at most n_scaf scaffolds and total is at most SEATS_MAX_TABLE: no product or sum overflows
        const int64_t members = seq_first[lift_seq[s] + 1] - seq_first[lift_seq[s]];
        if (n_seq > SEATS_MAX_TABLE || members > SEATS_MAX_TABLE / 4) return -1;
        const int64_t block = n_seq + 4 * members;
        if (block > SEATS_MAX_TABLE - total) return -1;
        first[s] = total;
        total += block;
    }
    return total;
}

// The resident pair store keeps no intra pair (pairs.h): one on a placed scaffold is SEATS_SAME, on a dropped one
// SEATS_UNLIFTED, under any ordering.
inline void seats_add_intra(const uint64_t* intra, const int32_t* lift_seq, int64_t n_scaf, uint64_t* counters5)
{
    for (int64_t s = 0; s < n_scaf; s++) counters5[lift_seq[s] >= 0 ? SEATS_SAME : SEATS_UNLIFTED] += intra[s];
}

}  // namespace hicmi
