// pairs_host_check.cpp - the kept mask and the counter sums of csrc/pairs.h as host code, with a compaction written on them,
// for a build with -fsanitize=address,undefined (tests/test_pairs_cpu.py writes the case file and compares the output with
// tests/pairs_reference.py).  Every array is a heap block of exactly its size, so a write past the store is reported.
//
// Case file, blank-separated:  S n_scaf | n_scaf x lift_seq | P n first | n x (sa pa sb pb).  The pairs are compacted in
// two calls, the first `first` of them and the rest, into a store of exactly as many pairs as are kept.  Output: per pair
// "keep <0|1>", "kept <n>", per kept pair "k <sa> <pa> <sb> <pb>", per scaffold "intra <count>", "sums <placed> <dropped>",
// "ends" and "anchor" with six counters each that started from 1 .. 6.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "pairs.h"

using namespace hicmi;

// The stable compaction of n pairs written out on the host with pairs_kept: the kept pairs in the order they come, appended
// from index `at` on to arrays with room for them, and intra[] counted.  Returns the new length.  It is this program's own
// restatement - the library compacts on the device only (k_pairs_keep) - so what the sanitizers check of the library's code
// is pairs_kept, pairs_intra_sums and the two pairs_add_intra_* functions.
static int64_t pairs_keep_host(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                               int64_t at, int32_t* keep_scaf_a, int64_t* keep_pos_a, int32_t* keep_scaf_b, int64_t* keep_pos_b,
                               uint64_t* intra)
{
    for (int64_t p = 0; p < n; p++) {
        if (!pairs_kept(scaf_a[p], scaf_b[p])) { intra[scaf_a[p]] += 1; continue; }
        keep_scaf_a[at] = scaf_a[p]; keep_pos_a[at] = pos_a[p];
        keep_scaf_b[at] = scaf_b[p]; keep_pos_b[at] = pos_b[p];
        at++;
    }
    return at;
}

static long long next_ll(FILE* fh)
{
    long long v;
    if (fscanf(fh, "%lld", &v) != 1) { fprintf(stderr, "short case file\n"); exit(2); }
    return v;
}

static void expect(FILE* fh, char tag)
{
    char got = 0;
    if (fscanf(fh, " %c", &got) != 1 || got != tag) { fprintf(stderr, "expected %c in the case file\n", tag); exit(2); }
}

int main(int argc, char** argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    FILE* fh = fopen(argv[1], "r");
    if (!fh) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    expect(fh, 'S');
    const int64_t n_scaf = next_ll(fh);
    std::unique_ptr<int32_t[]> seq(new int32_t[n_scaf]);
    for (int64_t s = 0; s < n_scaf; s++) seq[s] = (int32_t)next_ll(fh);
    expect(fh, 'P');
    const int64_t n = next_ll(fh), first = next_ll(fh);
    std::unique_ptr<int32_t[]> sa(new int32_t[n]), sb(new int32_t[n]);
    std::unique_ptr<int64_t[]> pa(new int64_t[n]), pb(new int64_t[n]);
    int64_t n_kept = 0;
    for (int64_t p = 0; p < n; p++) {
        sa[p] = (int32_t)next_ll(fh); pa[p] = next_ll(fh); sb[p] = (int32_t)next_ll(fh); pb[p] = next_ll(fh);
        const bool kept = pairs_kept(sa[p], sb[p]);
        printf("keep %d\n", kept ? 1 : 0);
        n_kept += kept;
    }
    fclose(fh);
    std::unique_ptr<int32_t[]> ka(new int32_t[n_kept]), kb(new int32_t[n_kept]);
    std::unique_ptr<int64_t[]> qa(new int64_t[n_kept]), qb(new int64_t[n_kept]);
    std::unique_ptr<uint64_t[]> intra(new uint64_t[n_scaf]());
    int64_t at = pairs_keep_host(sa.get(), pa.get(), sb.get(), pb.get(), first, 0, ka.get(), qa.get(), kb.get(), qb.get(), intra.get());
    at = pairs_keep_host(sa.get() + first, pa.get() + first, sb.get() + first, pb.get() + first, n - first, at, ka.get(), qa.get(), kb.get(),
                         qb.get(), intra.get());
    printf("kept %" PRId64 "\n", at);
    for (int64_t k = 0; k < at; k++) printf("k %d %" PRId64 " %d %" PRId64 "\n", ka[k], qa[k], kb[k], qb[k]);
    for (int64_t s = 0; s < n_scaf; s++) printf("intra %" PRIu64 "\n", intra[s]);
    uint64_t placed = 0, dropped = 0;
    pairs_intra_sums(intra.get(), seq.get(), n_scaf, &placed, &dropped);
    printf("sums %" PRIu64 " %" PRIu64 "\n", placed, dropped);
    uint64_t ends[ENDS_COUNTERS] = {1, 2, 3, 4, 5, 6}, anchor[ANCHOR_COUNTERS] = {1, 2, 3, 4, 5, 6};
    pairs_add_intra_ends(intra.get(), seq.get(), n_scaf, ends);
    pairs_add_intra_anchor(intra.get(), seq.get(), n_scaf, anchor);
    printf("ends");
    for (int k = 0; k < ENDS_COUNTERS; k++) printf(" %" PRIu64, ends[k]);
    printf("\nanchor");
    for (int k = 0; k < ANCHOR_COUNTERS; k++) printf(" %" PRIu64, anchor[k]);
    printf("\n");
    return 0;
}
