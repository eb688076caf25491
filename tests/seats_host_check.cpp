// seats_host_check.cpp - the blocks and the classification of a pair of csrc/seats.h as host code, for a build with
// -fsanitize=address,undefined (tests/test_seats_cpu.py writes the case file and compares the output with
// tests/seats_reference.py).  Every array is a heap block of exactly its size, so a read past a table is reported.
//
// Case file, blank-separated:  T n_scaf n_seq window print_table | n_scaf x (size seq off rev) | n_seq sizes | P n |
// n x (sa pa sb pb).  Output: "check <rc> <message>", "table <n>" (-1: past the limit), per scaffold "first <offset>", per
// pair "pair <kind> <i0> <i1> <i2> <i3>" (the counters it adds to, then -1), "counters" and the five of them, and with
// print_table per counter of the table "t <count>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "seats.h"

using namespace hicmi;

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
    expect(fh, 'T');
    const int64_t n_scaf = next_ll(fh), n_seq = next_ll(fh), window = next_ll(fh), print_table = next_ll(fh);
    std::unique_ptr<int64_t[]> size(new int64_t[n_scaf]), off(new int64_t[n_scaf]), seq_size(new int64_t[n_seq]), first(new int64_t[n_scaf]);
    std::unique_ptr<int64_t[]> seq_first(new int64_t[n_seq + 1]);
    std::unique_ptr<int32_t[]> seq(new int32_t[n_scaf]), rank(new int32_t[n_scaf]);
    std::unique_ptr<uint8_t[]> rev(new uint8_t[n_scaf]);
    for (int64_t s = 0; s < n_scaf; s++) {
        size[s] = next_ll(fh); seq[s] = (int32_t)next_ll(fh); off[s] = next_ll(fh); rev[s] = (uint8_t)next_ll(fh);
    }
    for (int64_t q = 0; q < n_seq; q++) seq_size[q] = next_ll(fh);
    char msg[256] = "";
    const int rc = lift_check_tables(size.get(), n_scaf, seq.get(), off.get(), rev.get(), seq_size.get(), n_seq, msg, sizeof(msg));
    printf("check %d %s\n", rc, msg);
    if (rc) return 0;
    if (ends_number_ranks(size.get(), n_scaf, seq.get(), off.get(), n_seq, 1, rank.get(), seq_first.get()) < 0) { printf("ranks -1\n"); return 0; }
    const int64_t n_table = seats_number_blocks(size.get(), n_scaf, seq.get(), n_seq, seq_first.get(), first.get());
    printf("table %" PRId64 "\n", n_table);
    if (n_table < 0) return 0;
    for (int64_t s = 0; s < n_scaf; s++) printf("first %" PRId64 "\n", first[s]);
    LiftTables L;
    L.seq = seq.get(); L.off = off.get(); L.rev = rev.get(); L.scaf_size = size.get();
    L.n_scaf = (int32_t)n_scaf; L.n_seq = (int32_t)n_seq;
    SeatsGrid G;
    G.first = first.get(); G.rank = rank.get(); G.seq_first = seq_first.get(); G.window = window;
    const int64_t m = print_table ? n_table : 0;
    std::unique_ptr<unsigned long long[]> T(new unsigned long long[m]());
    unsigned long long counters[SEATS_COUNTERS] = {0, 0, 0, 0, 0};
    expect(fh, 'P');
    const int64_t n_pairs = next_ll(fh);
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t sa = (int32_t)next_ll(fh); const int64_t pa = next_ll(fh);
        const int32_t sb = (int32_t)next_ll(fh); const int64_t pb = next_ll(fh);
        int64_t index[4] = {-1, -1, -1, -1};
        int n_index = 0;
        const int kind = seats_classify(L, G, sa, pa, sb, pb, index, &n_index);
        for (int k = 0; k < 4; k++) {
            if (k >= n_index) { index[k] = -1; continue; }
            if (index[k] < 0 || index[k] >= n_table) { fprintf(stderr, "pair %" PRId64 ": index %" PRId64 " outside the table\n", p, index[k]); return 3; }
            if (print_table) T[index[k]] += 1ull;
        }
        if (kind >= 0) counters[kind]++;
        printf("pair %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", kind, index[0], index[1], index[2], index[3]);
    }
    printf("counters");
    for (int k = 0; k < SEATS_COUNTERS; k++) printf(" %llu", counters[k]);
    printf("\n");
    for (int64_t k = 0; k < m; k++) printf("t %llu\n", T[k]);
    fclose(fh);
    return 0;
}
