// anchor.h - anchoring the scaffolds an ordering leaves out: the blocks of counters the candidates own, the
// kind of a pair and the counter an anchored pair adds to.  Like ends.h it is plain integer arithmetic without a GPU
// dependency: the kernels of k_anchor.hip and api.hip include it, and so does a stand-alone host program built with the
// sanitizers (tests/anchor_host_check.cpp).
#pragma once
#include "ends.h"

namespace hicmi {

constexpr int64_t ANCHOR_MAX_TABLE = (int64_t)1 << 27;    // counters of a table: the blocks of all candidates

// what a pair is to the table; the value is the index of its counter.  A pair is checked for PLACED, UNPLACED, SKIPPED,
// ELSEWHERE and MIDDLE in this order; what is left is ANCHORED.
enum AnchorKind { ANCHOR_ANCHORED = 0, ANCHOR_MIDDLE = 1, ANCHOR_ELSEWHERE = 2, ANCHOR_SKIPPED = 3, ANCHOR_UNPLACED = 4,
                  ANCHOR_PLACED = 5, ANCHOR_COUNTERS = 6, ANCHOR_NOWHERE = -1 };

// The blocks of a build (device memory in a kernel): first per scaffold (-1: no candidate); in rank mode the target
// sequence per scaffold, the rank per scaffold (ends_number_ranks) and seq_first[n_seq + 1]; target == nullptr is the
// sequence mode, which looks at neither rank nor seq_first nor window.
struct AnchorGrid {
    const int64_t* first = nullptr;
    const int32_t* target = nullptr;
    const int32_t* rank = nullptr;
    const int64_t* seq_first = nullptr;
    int64_t window = 1;
};

// The half of a candidate of length len the 1-based position p falls in, in the candidate's + coordinates: the first
// half takes the odd base.
LIFT_HD int anchor_half(int64_t len, int64_t p) { return p - 1 < len - len / 2 ? 0 : 1; }

// What the pair (sa, pa, sb, pb) is, and for ANCHOR_ANCHORED the index of its counter in the table.  Sequence mode:
// first[c] + q with c the dropped scaffold and q the sequence of the placed end.  Rank mode:
// first[c] + (r - seq_first[q]) * 4 + zu * 2 + zp with r the rank of the scaffold under the placed end, zu the half of c
// and zp the zone of the placed end as it lies.  ANCHOR_NOWHERE: an end outside the tables or its scaffold (the host
// refuses those before a chunk is uploaded).
template <bool RANK_MODE>
LIFT_HD int anchor_classify(const LiftTables& L, const AnchorGrid& G, int32_t sa, int64_t pa, int32_t sb, int64_t pb, int64_t* index_out)
{
    int32_t qa, qb;
    int64_t ya = 0, yb = 0;
    const bool ok_a = lift_end(L, sa, pa, &qa, &ya), ok_b = lift_end(L, sb, pb, &qb, &yb);
    if ((!ok_a && qa != -1) || (!ok_b && qb != -1)) return ANCHOR_NOWHERE;
    if (ok_a && ok_b) return ANCHOR_PLACED;
    if (!ok_a && !ok_b) return ANCHOR_UNPLACED;
    const int32_t c = ok_a ? sb : sa, s = ok_a ? sa : sb, q = ok_a ? qa : qb;      // c: the dropped one, s: the placed one
    const int64_t pc = ok_a ? pb : pa, ps = ok_a ? pa : pb;
    const int64_t first = G.first[c];
    if (first < 0) return ANCHOR_SKIPPED;
    if (!RANK_MODE) {
        *index_out = first + q;
        return ANCHOR_ANCHORED;
    }
    if (G.target[c] != q) return ANCHOR_ELSEWHERE;
    const int zp = ends_zone(L.scaf_size[s], ps, L.rev[s] != 0, G.window);
    if (zp == ENDS_MID) return ANCHOR_MIDDLE;
    const int64_t k = (int64_t)G.rank[s] - G.seq_first[q];
    if (G.rank[s] < 0 || k < 0 || k >= G.seq_first[q + 1] - G.seq_first[q]) return ANCHOR_NOWHERE;
    *index_out = first + k * 4 + anchor_half(L.scaf_size[c], pc) * 2 + zp;
    return ANCHOR_ANCHORED;
}

// The host's check of the targets of a rank-mode build against tables that passed lift_check_tables and the seq_first
// of ends_number_ranks.  0 when they are usable; else -1 and a message naming the scaffold.
inline int anchor_check_targets(const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, int64_t n_seq, const int32_t* target,
                                const int64_t* seq_first, char* msg, size_t msg_cap)
{
    for (int64_t s = 0; s < n_scaf; s++) {
        const int64_t t = target[s];
        if (t < -1 || t >= n_seq) {
            snprintf(msg, msg_cap, "scaffold %lld has the target %lld, outside -1 .. %lld", (long long)s, (long long)t, (long long)(n_seq - 1));
            return -1;
        }
        if (t < 0) continue;
        if (lift_seq[s] >= 0) {
            snprintf(msg, msg_cap, "scaffold %lld has a target but lies in sequence %d", (long long)s, lift_seq[s]);
            return -1;
        }
        if (scaf_size[s] <= 0) {
            snprintf(msg, msg_cap, "scaffold %lld has a target but no base", (long long)s);
            return -1;
        }
        if (seq_first[t + 1] == seq_first[t]) {
            snprintf(msg, msg_cap, "scaffold %lld has the target %lld, a sequence without a placed scaffold that has a base", (long long)s,
                     (long long)t);
            return -1;
        }
    }
    return 0;
}

// The blocks of a build on the host, from tables that passed lift_check_tables (and, in rank mode, targets that passed
// anchor_check_targets): the candidates in index order, each with a block of n_seq counters (target == nullptr) or of
// 4 x (placed scaffolds of its target sequence) counters.  first[n_scaf] (-1 for a scaffold that is no candidate).
// Returns the size of the table - 0: there is no candidate - or -1 as soon as it passes ANCHOR_MAX_TABLE.
inline int64_t anchor_number_blocks(const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, int64_t n_seq, const int32_t* target,
                                    const int64_t* seq_first, int64_t* first)
{
    int64_t total = 0;
    for (int64_t s = 0; s < n_scaf; s++) {
        first[s] = -1;
        if (lift_seq[s] >= 0 || scaf_size[s] <= 0 || (target && target[s] < 0)) continue;
        // a block has at most 4 x n_scaf or n_seq counters and total at most ANCHOR_MAX_TABLE: no product or sum overflows
        const int64_t block = target ? 4 * (seq_first[target[s] + 1] - seq_first[target[s]]) : n_seq;
        if (block > ANCHOR_MAX_TABLE - total) return -1;
        first[s] = total;
        total += block;
    }
    return total;
}

}  // namespace hicmi
