// span_host_check.cpp - the cell numbering, the classification of a pair, the competing slots and the pick of csrc/span.h as
// host code, for a build with -fsanitize=address,undefined (tests/test_spans_cpu.py writes the case file and compares the
// output with tests/span_reference.py).  Every array is a heap block of exactly its size, so a read past a table is reported.
//
// Case file, blank-separated:  T n_scaf n_seq step max_span flank | n_scaf x (size seq off rev) | n_seq sizes |
// P n | n x (sa pa sb pb) | R n | n x (lo hi q0 q1).  Output: "check <rc> <message>", "cells <n>" (-1: too many), per
// scaffold "first <cell>", per sequence and once more "seq <cell>", per pair "pair <kind> <lo> <hi>" (-1 -1 unless it
// marks), per cell "depth <D>", per record "pick <slot> <D> <Lsum> <Rsum> <ratio as %a, or NA>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "span.h"

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
    const int64_t n_scaf = next_ll(fh), n_seq = next_ll(fh), step = next_ll(fh), max_span = next_ll(fh), flank = next_ll(fh);
    std::unique_ptr<int64_t[]> size(new int64_t[n_scaf]), off(new int64_t[n_scaf]), seq_size(new int64_t[n_seq]);
    std::unique_ptr<int64_t[]> cell_first(new int64_t[n_scaf]), seq_first(new int64_t[n_seq + 1]);
    std::unique_ptr<int32_t[]> seq(new int32_t[n_scaf]);
    std::unique_ptr<uint8_t[]> rev(new uint8_t[n_scaf]);
    for (int64_t s = 0; s < n_scaf; s++) {
        size[s] = next_ll(fh); seq[s] = (int32_t)next_ll(fh); off[s] = next_ll(fh); rev[s] = (uint8_t)next_ll(fh);
    }
    for (int64_t q = 0; q < n_seq; q++) seq_size[q] = next_ll(fh);
    char msg[256] = "";
    const int rc = lift_check_tables(size.get(), n_scaf, seq.get(), off.get(), rev.get(), seq_size.get(), n_seq, msg, sizeof(msg));
    printf("check %d %s\n", rc, msg);
    if (rc) return 0;
    const int64_t m = span_number_cells(size.get(), n_scaf, seq.get(), off.get(), n_seq, step, cell_first.get(), seq_first.get());
    printf("cells %" PRId64 "\n", m);
    if (m < 0) return 0;
    for (int64_t s = 0; s < n_scaf; s++) printf("first %" PRId64 "\n", cell_first[s]);
    for (int64_t q = 0; q <= n_seq; q++) printf("seq %" PRId64 "\n", seq_first[q]);
    LiftTables L;
    L.seq = seq.get(); L.off = off.get(); L.rev = rev.get(); L.scaf_size = size.get();
    L.n_scaf = (int32_t)n_scaf; L.n_seq = (int32_t)n_seq;
    SpanGrid G;
    G.cell_first = cell_first.get(); G.step = step; G.max_span = max_span; G.n_cells = m;
    std::unique_ptr<unsigned long long[]> D(new unsigned long long[m]()), S(new unsigned long long[m]());
    expect(fh, 'P');
    const int64_t n_pairs = next_ll(fh);
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t sa = (int32_t)next_ll(fh); const int64_t pa = next_ll(fh);
        const int32_t sb = (int32_t)next_ll(fh); const int64_t pb = next_ll(fh);
        int64_t lo = -1, hi = -1;
        const int kind = span_classify(L, G, sa, pa, sb, pb, &lo, &hi);
        if (kind == SPAN_MARKED) { D[lo] += 1ull; D[hi] += ~0ull; }
        else lo = hi = -1;
        printf("pair %d %" PRId64 " %" PRId64 "\n", kind, lo, hi);
    }
    for (int64_t c = 1; c < m; c++) D[c] += D[c - 1];
    for (int64_t c = 0; c < m; c++) { S[c] = D[c] + (c ? S[c - 1] : 0ull); printf("depth %llu\n", D[c]); }
    expect(fh, 'R');
    const int64_t n_rec = next_ll(fh);
    for (int64_t r = 0; r < n_rec; r++) {
        const int64_t lo = next_ll(fh), hi = next_ll(fh), q0 = next_ll(fh), q1 = next_ll(fh);
        int64_t out4[4];
        span_pick(D.get(), S.get(), flank, lo, hi, q0, q1, out4);
        printf("pick %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " ", out4[0], out4[1], out4[2], out4[3]);
        if (out4[0] < 0) printf("NA\n");
        else printf("%a\n", span_ratio((unsigned long long)out4[1], flank, (unsigned long long)out4[2], (unsigned long long)out4[3]));
    }
    fclose(fh);
    return 0;
}
