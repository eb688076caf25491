// ends.h - end support: the ranks of the placed scaffolds, the zone of a read end on its scaffold, and the
// counter a pair between two neighbouring scaffolds adds to.  Like span.h it is plain integer arithmetic without a GPU
// dependency: the kernels of k_ends.hip and api.hip include it, and so does a stand-alone host program built with the
// sanitizers (tests/ends_host_check.cpp).
#pragma once
#include "liftmap.h"

namespace hicmi {

constexpr int64_t ENDS_MAX_TABLE = (int64_t)1 << 27;      // counters of a table: placed scaffolds x reach x 4
constexpr int64_t ENDS_MAX_REACH = 64;

// what a pair is to the table; the value is the index of its counter.  A pair is checked for UNLIFTED, TRANS, SAME,
// TOO_FAR and MIDDLE in this order; what is left is LINKED.
enum EndsKind { ENDS_LINKED = 0, ENDS_MIDDLE = 1, ENDS_SAME = 2, ENDS_TOO_FAR = 3, ENDS_TRANS = 4, ENDS_UNLIFTED = 5, ENDS_COUNTERS = 6,
                ENDS_NOWHERE = -1 };

enum EndsZone { ENDS_LEFT = 0, ENDS_RIGHT = 1, ENDS_MID = 2 };

// The ranks of a build: rank per scaffold (-1: dropped or empty; device memory in a kernel), the window in bases, the
// reach in ranks and the number of placed scaffolds.
struct EndsGrid {
    const int32_t* rank = nullptr;
    int64_t window = 1, reach = 1, n_placed = 0;
};

// The zones of a scaffold of length len at the window W >= 1, in bases: the left one and the right one as it lies.  A
// scaffold of up to 2 W bases is cut in halves, the left half taking the odd base.
LIFT_HD int64_t ends_left_zone(int64_t len, int64_t window) { const int64_t half = len - len / 2; return window < half ? window : half; }
LIFT_HD int64_t ends_right_zone(int64_t len, int64_t window) { const int64_t half = len / 2; return window < half ? window : half; }

// Zone of the 1-based position p on a scaffold of length len >= p: the lying coordinate is counted from the scaffold's
// left end as it lies in its sequence, which is its base len when it is reversed.
LIFT_HD int ends_zone(int64_t len, int64_t p, bool rev, int64_t window)
{
    const int64_t x = rev ? len - p : p - 1;
    if (x < ends_left_zone(len, window)) return ENDS_LEFT;
    if (x >= len - ends_right_zone(len, window)) return ENDS_RIGHT;
    return ENDS_MID;
}

// What the pair (sa, pa, sb, pb) is, and for ENDS_LINKED the index of its counter in the table:
// ((i * reach + (d - 1)) * 4 + za * 2 + zb) with i the lower rank, d the rank difference, za the zone of the end on the
// scaffold of rank i and zb the zone of the other end.  ENDS_NOWHERE: an end outside the tables or its scaffold (the host
// refuses those before a chunk is uploaded).
LIFT_HD int ends_classify(const LiftTables& L, const EndsGrid& G, int32_t sa, int64_t pa, int32_t sb, int64_t pb, int64_t* index_out)
{
    int32_t qa, qb;
    int64_t ya = 0, yb = 0;
    const bool ok_a = lift_end(L, sa, pa, &qa, &ya), ok_b = lift_end(L, sb, pb, &qb, &yb);
    if (!ok_a || !ok_b) return qa >= -1 && qb >= -1 ? ENDS_UNLIFTED : ENDS_NOWHERE;
    if (qa != qb) return ENDS_TRANS;
    if (sa == sb) return ENDS_SAME;
    const int64_t ra = G.rank[sa], rb = G.rank[sb];
    if (ra < 0 || rb < 0 || ra >= G.n_placed || rb >= G.n_placed || ra == rb) return ENDS_NOWHERE;
    const int64_t d = ra < rb ? rb - ra : ra - rb;
    if (d > G.reach) return ENDS_TOO_FAR;
    const int za = ends_zone(L.scaf_size[sa], pa, L.rev[sa] != 0, G.window);
    const int zb = ends_zone(L.scaf_size[sb], pb, L.rev[sb] != 0, G.window);
    if (za == ENDS_MID || zb == ENDS_MID) return ENDS_MIDDLE;
    const int64_t i = ra < rb ? ra : rb;
    *index_out = (i * G.reach + (d - 1)) * 4 + (ra < rb ? za * 2 + zb : zb * 2 + za);
    return ENDS_LINKED;
}

// The ranks of a build on the host, from tables that passed lift_check_tables: sequences ascending, inside a sequence
// the scaffolds by offset, then by index.  rank[n_scaf] (-1 for a dropped or empty scaffold), seq_first[n_seq + 1] (the
// scaffolds of sequence q have the ranks [seq_first[q], seq_first[q + 1])).  Returns the number of placed scaffolds P,
// or -1 as soon as P x reach x 4 passes ENDS_MAX_TABLE.  reach must lie in 1 .. ENDS_MAX_REACH.
inline int64_t ends_number_ranks(const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                                 int64_t n_seq, int64_t reach, int32_t* rank, int64_t* seq_first)
{
    std::vector<int64_t> placed;
    for (int64_t s = 0; s < n_scaf; s++) {
        rank[s] = -1;
        if (lift_seq[s] >= 0 && scaf_size[s] > 0) placed.push_back(s);
    }
    std::sort(placed.begin(), placed.end(), [&](int64_t a, int64_t b) {
        if (lift_seq[a] != lift_seq[b]) return lift_seq[a] < lift_seq[b];
        if (lift_off[a] != lift_off[b]) return lift_off[a] < lift_off[b];
        return a < b;
    });
    const int64_t most = ENDS_MAX_TABLE / 4 / reach;          // P x reach x 4 <= ENDS_MAX_TABLE, without the product
    int64_t n = 0, q = 0;
    seq_first[0] = 0;
    for (const int64_t s : placed) {
        while (q < lift_seq[s]) seq_first[++q] = n;
        if (n >= most) return -1;
        rank[s] = (int32_t)n++;
    }
    while (q < n_seq) seq_first[++q] = n;
    return n;
}

}  // namespace hicmi
