// liftmap.h - the lift of a read end from (scaffold, position) to (assembled sequence, position), the key of the cell a
// pair counts in, the contact-decay slot, and the host's check of the lift tables.  Everything here is plain integer
// arithmetic without a GPU dependency: the kernels of k_buildmap.hip and api.hip include it, and so does a stand-alone
// host program built with the sanitizers (tests/liftmap_host_check.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define LIFT_HD __host__ __device__ __forceinline__
#else
#define LIFT_HD inline
#endif

namespace hicmi {

// Per scaffold: the sequence it lies in (-1: dropped), its offset there and whether it is reversed; scaf_size as in the
// size file.  The pointers are device memory in a kernel and host memory in the check.  seq == nullptr: no lift.
struct LiftTables {
    const int32_t* seq = nullptr;
    const int64_t* off = nullptr;
    const uint8_t* rev = nullptr;
    const int64_t* scaf_size = nullptr;
    int32_t n_scaf = 0, n_seq = 0;
};

constexpr int LIFT_DECAY_SLOTS = 256;

constexpr unsigned long long kNoKey = ~0ull;      // lo * m + hi <= 2^32 - 1 for m <= 65536

// The key lo * m + hi of the cell a pair counts in, or kNoKey for a pair outside the map.  Its ends are the 1-based
// positions xa and xb on the grid elements ga and gb: scaffolds or, after the lift, assembled sequences.
// Element g has its bins from first_bin[g] on, cut from its own start at bin size r.
LIFT_HD unsigned long long map_cell_key(int32_t ga, int64_t xa, int32_t gb, int64_t xb, const int32_t* first_bin, int n_grid,
                                         int64_t r, int m)
{
    const int64_t pa = xa - 1, pb = xb - 1;
    if (ga < 0 || ga >= n_grid || gb < 0 || gb >= n_grid || pa < 0 || pb < 0) return kNoKey;
    int64_t ka, kb;
    if (((uint64_t)pa | (uint64_t)pb | (uint64_t)r) >> 32) { ka = pa / r; kb = pb / r; }
    else { ka = (uint32_t)pa / (uint32_t)r; kb = (uint32_t)pb / (uint32_t)r; }      // the usual case: 32-bit division
    const int64_t i = first_bin[ga] + ka, j = first_bin[gb] + kb;
    if (i >= m || j >= m) return kNoKey;
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
    return (unsigned long long)(lo * m + hi);
}

// The 1-based position p on scaffold s, lifted: off + p, or off + L - p + 1 on a reversed scaffold.  false for an end
// outside the tables or outside its scaffold, and for a dropped scaffold (*seq_out = -1 then tells the two apart).
LIFT_HD bool lift_end(const LiftTables& L, int32_t s, int64_t p, int32_t* seq_out, int64_t* pos_out)
{
    *seq_out = -2;
    if (s < 0 || s >= L.n_scaf) return false;
    const int64_t len = L.scaf_size[s];
    if (p < 1 || p > len) return false;
    const int32_t q = L.seq[s];
    *seq_out = q < 0 ? -1 : q;
    if (q < 0 || q >= L.n_seq) return false;
    *pos_out = L.off[s] + (L.rev[s] ? len - p + 1 : p);
    return true;
}

// Slot of the distance d in the contact-decay histogram: 0 for d = 0, else quarter octaves,
// 1 + 4 e + (((d - 2^e) * 4) >> e) with e = floor(log2 d).  From e = 2 on the product is written as a shift by e - 2,
// which is the same integer and cannot overflow at e = 62.
LIFT_HD int lift_decay_slot(uint64_t d)
{
    if (d == 0) return 0;
    const int e = 63 - __builtin_clzll((unsigned long long)d);
    const uint64_t x = d - ((uint64_t)1 << e);
    const uint64_t quarter = e >= 2 ? x >> (e - 2) : (x * 4) >> e;
    return 1 + 4 * e + (int)quarter;
}

// The host's check of the tables of one lifted build.  0 when they are usable; else -1 and a message naming the scaffold.
inline int lift_check_tables(const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                             const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, char* msg, size_t msg_cap)
{
    (void)lift_rev;
    for (int64_t q = 0; q < n_seq; q++)
        if (seq_size[q] < 0) {
            snprintf(msg, msg_cap, "sequence %lld has the negative size %lld", (long long)q, (long long)seq_size[q]);
            return -1;
        }
    std::vector<int64_t> placed;
    for (int64_t s = 0; s < n_scaf; s++) {
        if (scaf_size[s] < 0) {
            snprintf(msg, msg_cap, "scaffold %lld has the negative size %lld", (long long)s, (long long)scaf_size[s]);
            return -1;
        }
        if (lift_seq[s] < -1 || lift_seq[s] >= n_seq) {
            snprintf(msg, msg_cap, "scaffold %lld lies in sequence %d, outside -1 .. %lld", (long long)s, lift_seq[s],
                     (long long)(n_seq - 1));
            return -1;
        }
        if (lift_seq[s] < 0) continue;
        if (lift_off[s] < 0) {
            snprintf(msg, msg_cap, "scaffold %lld has the negative offset %lld", (long long)s, (long long)lift_off[s]);
            return -1;
        }
        const int64_t room = seq_size[lift_seq[s]];
        if (scaf_size[s] > room || lift_off[s] > room - scaf_size[s]) {        // off + size > room, without the sum
            snprintf(msg, msg_cap, "scaffold %lld (offset %lld, size %lld) ends beyond its sequence %d of size %lld", (long long)s,
                     (long long)lift_off[s], (long long)scaf_size[s], lift_seq[s], (long long)room);
            return -1;
        }
        if (scaf_size[s] > 0) placed.push_back(s);
    }
    std::sort(placed.begin(), placed.end(), [&](int64_t a, int64_t b) {
        if (lift_seq[a] != lift_seq[b]) return lift_seq[a] < lift_seq[b];
        if (lift_off[a] != lift_off[b]) return lift_off[a] < lift_off[b];
        return a < b;
    });
    for (size_t k = 1; k < placed.size(); k++) {
        const int64_t a = placed[k - 1], b = placed[k];
        if (lift_seq[a] == lift_seq[b] && lift_off[a] + scaf_size[a] > lift_off[b]) {
            snprintf(msg, msg_cap, "scaffolds %lld and %lld overlap in sequence %d", (long long)a, (long long)b, lift_seq[a]);
            return -1;
        }
    }
    return 0;
}

}  // namespace hicmi
