// split.h - scaffolds cut into pieces: the piece a read end falls in, what a pair adds to the counters of
// its pieces, and the host's check of the piece tables.  Like span.h it is plain integer arithmetic without a GPU
// dependency: the kernel of k_split.hip, api.hip and loader.hip include it, and so does a stand-alone host program built
// with the sanitizers (tests/split_host_check.cpp).
#pragma once
#include "liftmap.h"

namespace hicmi {

// Scaffold s of the size file has the pieces [piece_first[s], piece_first[s + 1]), left to right; piece k starts after
// piece_start[k] bases of its parent (0 for a first piece).  The pointers are device memory in a kernel.
struct SplitTables {
    const int32_t* piece_first = nullptr;   // [n_scaf + 1], ascending from 0 to n_piece
    const int64_t* piece_start = nullptr;   // [n_piece]
    int32_t n_scaf = 0, n_piece = 0;
};

// the four counters of a piece; counter `kind` of piece k is element kind * n_piece + k
enum SplitKind { SPLIT_WITHIN = 0, SPLIT_SIBLING = 1, SPLIT_OTHER = 2, SPLIT_MARK = 3, SPLIT_COUNTERS = 4 };

// The piece of the 1-based position p on scaffold s, 1 <= p <= size[s]: the last piece k of the scaffold with
// piece_start[k] < p; *pos_out = p - piece_start[k].  An uncut scaffold is its one piece; else a binary search.
LIFT_HD int32_t split_end(const SplitTables& T, int32_t s, int64_t p, int64_t* pos_out)
{
    int32_t lo = T.piece_first[s], hi = T.piece_first[s + 1];
    if (hi - lo > 1) {
        // piece_start[lo] = 0 < p holds throughout; piece_start[hi] >= p or hi is the scaffold's end
        while (hi - lo > 1) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (T.piece_start[mid] < p) lo = mid; else hi = mid;
        }
        p -= T.piece_start[lo];
    }
    *pos_out = p;
    return lo;
}

// The same, as the definition reads: a scan over the pieces of the scaffold
LIFT_HD int32_t split_end_scan(const SplitTables& T, int32_t s, int64_t p, int64_t* pos_out)
{
    int32_t k = T.piece_first[s];
    for (int32_t q = k + 1; q < T.piece_first[s + 1]; q++)
        if (T.piece_start[q] < p) k = q;
    *pos_out = p - T.piece_start[k];
    return k;
}

// What the pair with the ends in the pieces ka of scaffold sa and kb of scaffold sb adds: up to four counters idx[] get
// the amounts add[] (+1, or -1 for the mark at the higher piece); returns how many.
//   one piece                      within[ka] + 1
//   two pieces of one scaffold     sibling + 1 at both, mark + 1 at the lower and - 1 at the higher piece
//   pieces of two scaffolds        other + 1 at both
// The prefix sum of the marks over the pieces of a scaffold is, at piece k, the number of pairs with one end at or before
// the last base of k and one after it.
LIFT_HD int split_contributions(int64_t n_piece, int32_t sa, int32_t ka, int32_t sb, int32_t kb, int64_t* idx, int* add)
{
    if (ka == kb) { idx[0] = SPLIT_WITHIN * n_piece + ka; add[0] = 1; return 1; }
    if (sa != sb) {
        idx[0] = SPLIT_OTHER * n_piece + ka; idx[1] = SPLIT_OTHER * n_piece + kb;
        add[0] = add[1] = 1;
        return 2;
    }
    idx[0] = SPLIT_SIBLING * n_piece + ka; idx[1] = SPLIT_SIBLING * n_piece + kb;
    idx[2] = SPLIT_MARK * n_piece + (ka < kb ? ka : kb); idx[3] = SPLIT_MARK * n_piece + (ka < kb ? kb : ka);
    add[0] = add[1] = add[2] = 1; add[3] = -1;
    return 4;
}

// The host's check of the tables.  0 when they are usable; else -1 and a message naming the scaffold.
inline int split_check_tables(const int64_t* scaf_size, int64_t n_scaf, const int32_t* piece_first, const int64_t* piece_start,
                              int64_t n_piece, char* msg, size_t msg_cap)
{
    if (piece_first[0] != 0) {
        snprintf(msg, msg_cap, "scaffold 0 starts at piece %d, not at piece 0", piece_first[0]);
        return -1;
    }
    for (int64_t s = 0; s < n_scaf; s++) {
        const int64_t first = piece_first[s], last = piece_first[s + 1];
        if (scaf_size[s] < 0) {
            snprintf(msg, msg_cap, "scaffold %lld has the negative size %lld", (long long)s, (long long)scaf_size[s]);
            return -1;
        }
        if (last <= first || last > n_piece) {
            snprintf(msg, msg_cap, "scaffold %lld has the pieces %lld .. %lld: not one or more of the %lld pieces", (long long)s,
                     (long long)first, (long long)last - 1, (long long)n_piece);
            return -1;
        }
        if (scaf_size[s] == 0 && last - first != 1) {
            snprintf(msg, msg_cap, "scaffold %lld has no base and %lld pieces", (long long)s, (long long)(last - first));
            return -1;
        }
        if (piece_start[first] != 0) {
            snprintf(msg, msg_cap, "the first piece of scaffold %lld starts after %lld bases, not after 0", (long long)s,
                     (long long)piece_start[first]);
            return -1;
        }
        for (int64_t k = first + 1; k < last; k++)
            if (piece_start[k] <= piece_start[k - 1] || piece_start[k] >= scaf_size[s]) {
                snprintf(msg, msg_cap, "piece %lld of scaffold %lld (size %lld) starts after %lld bases: the starts must ascend below the size",
                         (long long)(k - first), (long long)s, (long long)scaf_size[s], (long long)piece_start[k]);
                return -1;
            }
    }
    if (piece_first[n_scaf] != n_piece) {
        snprintf(msg, msg_cap, "scaffold %lld ends at piece %d of %lld", (long long)(n_scaf - 1), piece_first[n_scaf], (long long)n_piece);
        return -1;
    }
    return 0;
}

}  // namespace hicmi
