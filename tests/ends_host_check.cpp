// ends_host_check.cpp - the ranks, the zones and the classification of a pair of csrc/ends.h as host code, for a build with
// -fsanitize=address,undefined (tests/test_ends_cpu.py writes the case file and compares the output with
// tests/ends_reference.py).  Every array is a heap block of exactly its size, so a read past a table is reported.
//
// Case file, blank-separated:  T n_scaf n_seq window reach print_table | n_scaf x (size seq off rev) | n_seq sizes |
// P n | n x (sa pa sb pb).  Output: "check <rc> <message>", "placed <P>" (-1: the table is past the limit), per scaffold
// "rank <r>", per sequence and once more "seq <r>", per pair "pair <kind> <index>" (-1 unless it is linked), "counters"
// and the six of them, and with print_table per counter of the table "t <count>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "ends.h"

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
    const int64_t n_scaf = next_ll(fh), n_seq = next_ll(fh), window = next_ll(fh), reach = next_ll(fh), print_table = next_ll(fh);
    std::unique_ptr<int64_t[]> size(new int64_t[n_scaf]), off(new int64_t[n_scaf]), seq_size(new int64_t[n_seq]);
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
    const int64_t P = ends_number_ranks(size.get(), n_scaf, seq.get(), off.get(), n_seq, reach, rank.get(), seq_first.get());
    printf("placed %" PRId64 "\n", P);
    if (P < 0) return 0;
    for (int64_t s = 0; s < n_scaf; s++) printf("rank %d\n", rank[s]);
    for (int64_t q = 0; q <= n_seq; q++) printf("seq %" PRId64 "\n", seq_first[q]);
    LiftTables L;
    L.seq = seq.get(); L.off = off.get(); L.rev = rev.get(); L.scaf_size = size.get();
    L.n_scaf = (int32_t)n_scaf; L.n_seq = (int32_t)n_seq;
    EndsGrid G;
    G.rank = rank.get(); G.window = window; G.reach = reach; G.n_placed = P;
    const int64_t m = print_table ? P * reach * 4 : 0;
    std::unique_ptr<unsigned long long[]> T(new unsigned long long[m]());
    unsigned long long counters[ENDS_COUNTERS] = {0, 0, 0, 0, 0, 0};
    expect(fh, 'P');
    const int64_t n_pairs = next_ll(fh);
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t sa = (int32_t)next_ll(fh); const int64_t pa = next_ll(fh);
        const int32_t sb = (int32_t)next_ll(fh); const int64_t pb = next_ll(fh);
        int64_t index = -1;
        const int kind = ends_classify(L, G, sa, pa, sb, pb, &index);
        if (kind != ENDS_LINKED) index = -1;
        else if (print_table) T[index] += 1ull;
        if (kind >= 0) counters[kind]++;
        printf("pair %d %" PRId64 "\n", kind, index);
    }
    printf("counters");
    for (int k = 0; k < ENDS_COUNTERS; k++) printf(" %llu", counters[k]);
    printf("\n");
    for (int64_t k = 0; k < m; k++) printf("t %llu\n", T[k]);
    fclose(fh);
    return 0;
}
