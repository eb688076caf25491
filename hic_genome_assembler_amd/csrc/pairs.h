// pairs.h - the resident pair store: which pairs are kept, what the others add to, and the counters an
// intra pair lands in under any ordering.  Like ends.h and anchor.h it is plain integer arithmetic without a GPU
// dependency: the kernels of k_pairs.hip and api.hip include it, and so does a stand-alone host program built with the
// sanitizers (tests/pairs_host_check.cpp), which checks these functions; the compaction itself exists on the device only.
#pragma once
#include "anchor.h"

namespace hicmi {

constexpr int64_t PAIRS_FIRST_PAIRS = (int64_t)1 << 22;   // the first capacity of a store (HICMI_PAIRS_FIRST_PAIRS)

// A pair is kept when its ends lie on two scaffolds.  A pair with both ends on one scaffold s is intra: it is not stored
// and adds 1 to intra[s].
LIFT_HD bool pairs_kept(int32_t sa, int32_t sb) { return sa != sb; }

// No ordering counts an intra pair in a table: it only lands in a kind counter, and which one follows from whether its
// scaffold is placed.  The sums of intra[] over the placed scaffolds (lift_seq >= 0) and over the dropped ones.
inline void pairs_intra_sums(const uint64_t* intra, const int32_t* lift_seq, int64_t n_scaf, uint64_t* placed_out, uint64_t* dropped_out)
{
    uint64_t placed = 0, dropped = 0;
    for (int64_t s = 0; s < n_scaf; s++) (lift_seq[s] >= 0 ? placed : dropped) += intra[s];
    *placed_out = placed; *dropped_out = dropped;
}

// ends_classify: an intra pair on a placed scaffold is ENDS_SAME, on a dropped one ENDS_UNLIFTED
inline void pairs_add_intra_ends(const uint64_t* intra, const int32_t* lift_seq, int64_t n_scaf, uint64_t* counters6)
{
    uint64_t placed, dropped;
    pairs_intra_sums(intra, lift_seq, n_scaf, &placed, &dropped);
    counters6[ENDS_SAME] += placed; counters6[ENDS_UNLIFTED] += dropped;
}

// anchor_classify, either mode: an intra pair on a placed scaffold is ANCHOR_PLACED, on a dropped one ANCHOR_UNPLACED
inline void pairs_add_intra_anchor(const uint64_t* intra, const int32_t* lift_seq, int64_t n_scaf, uint64_t* counters6)
{
    uint64_t placed, dropped;
    pairs_intra_sums(intra, lift_seq, n_scaf, &placed, &dropped);
    counters6[ANCHOR_PLACED] += placed; counters6[ANCHOR_UNPLACED] += dropped;
}

}  // namespace hicmi
