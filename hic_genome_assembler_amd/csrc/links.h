// links.h - the end-link graph of all scaffolds: the zone of a read end on its scaffold without any
// ordering, the key of a pair between two scaffolds, its kind, the hash of a key and the size of the find-or-insert table.
// Like ends.h and seats.h it is plain integer arithmetic without a GPU dependency: the kernels of k_links.hip and api.hip
// include it, and so does a stand-alone host program built with the sanitizers (tests/links_host_check.cpp).
#pragma once
#include "ends.h"

namespace hicmi {

constexpr int64_t LINKS_MAX_SCAF = (int64_t)1 << 30;      // scaffolds of a call: a key is then never the empty mark
constexpr int64_t LINKS_MIN_SLOTS = 1024;                 // slots of the smallest table
constexpr int64_t LINKS_MAX_SLOTS = (int64_t)1 << 31;     // slots of the largest one
constexpr uint64_t LINKS_EMPTY = ~(uint64_t)0;            // the key of a free slot

// the end combination of a pair: zone on the scaffold of lower index x 2 + zone on the other one; OTHER: an end in a
// middle zone.  The value is the low three bits of the key and the column of the row.
enum LinksCombo { LINKS_LL = 0, LINKS_LR = 1, LINKS_RL = 2, LINKS_RR = 3, LINKS_OTHER = 4, LINKS_COMBOS = 5 };

// what a stored pair is to the counters; NOWHERE: a pair the store never holds (one scaffold, or one outside the sizes)
enum LinksKind { LINKS_LINKED = 0, LINKS_MIDDLE = 1, LINKS_COUNTERS = 2, LINKS_NOWHERE = -1 };

LIFT_HD uint64_t links_key(int64_t lo, int64_t hi, int combo) { return (uint64_t)lo << 33 | (uint64_t)hi << 3 | (uint64_t)combo; }
LIFT_HD int64_t links_key_lo(uint64_t key) { return (int64_t)(key >> 33); }
LIFT_HD int64_t links_key_hi(uint64_t key) { return (int64_t)((key >> 3) & (((uint64_t)1 << 30) - 1)); }
LIFT_HD int links_key_combo(uint64_t key) { return (int)(key & 7u); }

// The kind of the pair (sa, pa, sb, pb) and its key.  A scaffold is read in its own + coordinates: the zones are those of
// ends_zone without a reversal, so ends_left_zone and ends_right_zone apply unchanged.
LIFT_HD int links_classify(const int64_t* scaf_size, int64_t n_scaf, int32_t sa, int64_t pa, int32_t sb, int64_t pb, int64_t window,
                           uint64_t* key_out)
{
    if (sa < 0 || sb < 0 || sa >= n_scaf || sb >= n_scaf || sa == sb) return LINKS_NOWHERE;
    const int za = ends_zone(scaf_size[sa], pa, false, window), zb = ends_zone(scaf_size[sb], pb, false, window);
    const bool a_low = sa < sb;
    const int zlo = a_low ? za : zb, zhi = a_low ? zb : za;
    const int combo = zlo == ENDS_MID || zhi == ENDS_MID ? LINKS_OTHER : zlo * 2 + zhi;
    *key_out = links_key(a_low ? sa : sb, a_low ? sb : sa, combo);
    return combo == LINKS_OTHER ? LINKS_MIDDLE : LINKS_LINKED;
}

// what a stored pair is to the counters of a count on lifted ends, checked in the order UNLIFTED, INSIDE,
// MIDDLE; what is left is LINKED.  The first two values are those of LinksKind.
enum LinksLiftedKind { LINKS_LIFTED_LINKED = 0, LINKS_LIFTED_MIDDLE = 1, LINKS_LIFTED_INSIDE = 2, LINKS_LIFTED_UNLIFTED = 3,
                       LINKS_LIFTED_COUNTERS = 4, LINKS_LIFTED_NOWHERE = -1 };

// The kind of the pair (sa, pa, sb, pb) between the ends of sequences that consist of several scaffolds, and for LINKED and
// MIDDLE its key.  Both ends are lifted (liftmap.h); an end on a dropped scaffold makes the pair UNLIFTED, two ends in one
// sequence make it INSIDE.  The zone of an end is that of its lifted 1-based position on its sequence read left to right:
// the bases of a gap belong to a zone and hold no read.  The key is that of the sequences in index order.  NOWHERE: a pair
// the store never holds (one scaffold, or an end outside the tables or its scaffold).
LIFT_HD int links_classify_lifted(const LiftTables& L, const int64_t* seq_size, int32_t sa, int64_t pa, int32_t sb, int64_t pb,
                                  int64_t window, uint64_t* key_out)
{
    if (sa == sb) return LINKS_LIFTED_NOWHERE;
    int32_t qa, qb;
    int64_t ya = 0, yb = 0;
    const bool ok_a = lift_end(L, sa, pa, &qa, &ya), ok_b = lift_end(L, sb, pb, &qb, &yb);
    if (!ok_a || !ok_b) return qa >= -1 && qb >= -1 ? LINKS_LIFTED_UNLIFTED : LINKS_LIFTED_NOWHERE;
    if (qa == qb) return LINKS_LIFTED_INSIDE;
    const int za = ends_zone(seq_size[qa], ya, false, window), zb = ends_zone(seq_size[qb], yb, false, window);
    const bool a_low = qa < qb;
    const int zlo = a_low ? za : zb, zhi = a_low ? zb : za;
    const int combo = zlo == ENDS_MID || zhi == ENDS_MID ? LINKS_OTHER : zlo * 2 + zhi;
    *key_out = links_key(a_low ? qa : qb, a_low ? qb : qa, combo);
    return combo == LINKS_OTHER ? LINKS_LIFTED_MIDDLE : LINKS_LIFTED_LINKED;
}

// The slot a key starts its probe sequence at in a table of 2^bits slots (1 <= bits <= 63): the high bits of the product
// with 2^64 / phi, so that the consecutive keys of one scaffold pair and of neighbouring scaffolds spread over the table.
LIFT_HD uint64_t links_slot(uint64_t key, int bits) { return (key * 0x9E3779B97F4A7C15ull) >> (64 - bits); }

// The keys a call can see at the most: min(n_kept, 5 n_scaf (n_scaf - 1) / 2).  n_scaf <= 2^30: the product stays below 2^62.
inline int64_t links_most_keys(int64_t n_kept, int64_t n_scaf)
{
    if (n_kept <= 0 || n_scaf < 2) return 0;
    const int64_t pairs = n_scaf % 2 ? n_scaf * ((n_scaf - 1) / 2) : (n_scaf / 2) * (n_scaf - 1);
    const int64_t keys = 5 * pairs;
    return n_kept < keys ? n_kept : keys;
}

// Slots of the table: the smallest power of two that is at least LINKS_MIN_SLOTS and at least twice links_most_keys, so the
// table is never more than half full and never grows.  The caller refuses a result above LINKS_MAX_SLOTS; *bits_out is
// its logarithm.  most <= 2^61 here, or the result saturates at 2^62.
inline int64_t links_capacity(int64_t n_kept, int64_t n_scaf, int* bits_out)
{
    const int64_t most = links_most_keys(n_kept, n_scaf);
    int bits = 10;
    while (bits < 62 && ((int64_t)1 << bits) / 2 < most) bits++;
    if (bits_out) *bits_out = bits;
    return (int64_t)1 << bits;
}

// The records (key, count) of the used slots sorted by key, in place: the slot order is the race's, and a key is (lo, hi,
// combination) from the top bit down.  A least-significant-digit radix sort with digits of 11 bits; a digit that all
// records share - the bits between hi and lo, the bits above lo - sorts nothing and is skipped, so 1,228 scaffolds take
// three passes.  Stable, and the keys of a table are distinct anyway.  Host only.
struct LinksRecord { uint64_t key, count; };
inline void links_sort_records(uint64_t* key, uint64_t* count, int64_t n_rec)
{
    if (n_rec < 2) return;
    constexpr int kDigit = 11;
    constexpr uint64_t kMask = ((uint64_t)1 << kDigit) - 1;
    std::vector<LinksRecord> a((size_t)n_rec), b((size_t)n_rec);
    for (int64_t r = 0; r < n_rec; r++) a[(size_t)r] = LinksRecord{key[r], count[r]};
    std::vector<int64_t> first((size_t)kMask + 1);
    for (int shift = 0; shift < 64; shift += kDigit) {
        std::fill(first.begin(), first.end(), (int64_t)0);
        for (const LinksRecord& x : a) first[(size_t)((x.key >> shift) & kMask)]++;
        if (first[(size_t)((a[0].key >> shift) & kMask)] == n_rec) continue;
        int64_t before = 0;
        for (int64_t& f : first) { const int64_t here = f; f = before; before += here; }
        for (const LinksRecord& x : a) b[(size_t)first[(size_t)((x.key >> shift) & kMask)]++] = x;
        a.swap(b);
    }
    for (int64_t r = 0; r < n_rec; r++) { key[r] = a[(size_t)r].key; count[r] = a[(size_t)r].count; }
}

// One row of the result per scaffold pair: the records (key, count) sorted by key are merged in place of a table.
// lo, hi: n_rows entries; counts5: n_rows x 5.  Returns the number of rows; the arrays have room for n_rec of them.
inline int64_t links_merge_rows(const uint64_t* key, const uint64_t* count, int64_t n_rec, int32_t* lo, int32_t* hi, uint64_t* counts5)
{
    int64_t n_rows = 0;
    for (int64_t r = 0; r < n_rec; r++) {
        const int32_t a = (int32_t)links_key_lo(key[r]), b = (int32_t)links_key_hi(key[r]);
        const int combo = links_key_combo(key[r]);
        if (combo >= LINKS_COMBOS) continue;                       // no key of links_classify
        if (n_rows == 0 || lo[n_rows - 1] != a || hi[n_rows - 1] != b) {
            lo[n_rows] = a; hi[n_rows] = b;
            for (int k = 0; k < LINKS_COMBOS; k++) counts5[n_rows * LINKS_COMBOS + k] = 0;
            n_rows++;
        }
        counts5[(n_rows - 1) * LINKS_COMBOS + combo] += count[r];
    }
    return n_rows;
}

}  // namespace hicmi
