// split_host_check.cpp - the table check, the piece of a read end in both forms and the counters of csrc/split.h as host
// code, for a build with -fsanitize=address,undefined (tests/test_split_cpu.py writes the case file and compares the output
// with tests/split_reference.py).  Every array is a heap block of exactly its size, so a read past a table is reported.
//
// Case file, blank-separated:  T n_scaf n_piece | n_scaf sizes | n_scaf + 1 x piece_first | n_piece x piece_start |
// P n | n x (sa pa sb pb).  Output: "check <rc> <message>" and, when the tables are usable, per pair
// "pair <piece a> <position a> <piece b> <position b>" (the bisection; "scan ..." follows where the scan gives another
// answer) and per counter, [within][sibling][other][mark] x n_piece, "counter <value>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "split.h"

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
    const int64_t n_scaf = next_ll(fh), n_piece = next_ll(fh);
    std::unique_ptr<int64_t[]> size(new int64_t[n_scaf]), start(new int64_t[n_piece]);
    std::unique_ptr<int32_t[]> first(new int32_t[n_scaf + 1]);
    for (int64_t s = 0; s < n_scaf; s++) size[s] = next_ll(fh);
    for (int64_t s = 0; s <= n_scaf; s++) first[s] = (int32_t)next_ll(fh);
    for (int64_t k = 0; k < n_piece; k++) start[k] = next_ll(fh);
    char msg[256] = "";
    const int rc = split_check_tables(size.get(), n_scaf, first.get(), start.get(), n_piece, msg, sizeof(msg));
    printf("check %d %s\n", rc, msg);
    if (rc) { fclose(fh); return 0; }
    SplitTables T;
    T.piece_first = first.get(); T.piece_start = start.get(); T.n_scaf = (int32_t)n_scaf; T.n_piece = (int32_t)n_piece;
    std::unique_ptr<unsigned long long[]> counters(new unsigned long long[SPLIT_COUNTERS * n_piece]());
    expect(fh, 'P');
    const int64_t n = next_ll(fh);
    for (int64_t p = 0; p < n; p++) {
        const int32_t sa = (int32_t)next_ll(fh);
        const int64_t pa = next_ll(fh);
        const int32_t sb = (int32_t)next_ll(fh);
        const int64_t pb = next_ll(fh);
        int64_t xa, xb, ya, yb;
        const int32_t ka = split_end(T, sa, pa, &xa), kb = split_end(T, sb, pb, &xb);
        const int32_t la = split_end_scan(T, sa, pa, &ya), lb = split_end_scan(T, sb, pb, &yb);
        printf("pair %d %" PRId64 " %d %" PRId64 "\n", ka, xa, kb, xb);
        if (la != ka || lb != kb || ya != xa || yb != xb) printf("scan %d %" PRId64 " %d %" PRId64 "\n", la, ya, lb, yb);
        int64_t idx[4];
        int add[4];
        const int m = split_contributions(n_piece, sa, ka, sb, kb, idx, add);
        for (int q = 0; q < m; q++) counters[idx[q]] += (unsigned long long)(long long)add[q];
    }
    for (int64_t q = 0; q < SPLIT_COUNTERS * n_piece; q++) printf("counter %llu\n", counters[q]);
    fclose(fh);
    return 0;
}
