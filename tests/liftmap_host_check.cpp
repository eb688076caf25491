// liftmap_host_check.cpp - the lift, the cell key, the decay slot and the table check of csrc/liftmap.h as host code, for a
// build with -fsanitize=address,undefined (tests/test_liftmap_cpu.py writes the case file and compares the output with
// tests/liftmap_reference.py).  Every array is a heap block of exactly its size, so a read past a table is reported.
//
// Case file, blank-separated:  T n_scaf n_seq r | n_scaf x (size seq off rev) | n_seq sizes | P n | n x (sa pa sb pb) |
// D n | n distances.  Output: "check <rc> <message>", per pair "pair qa xa qb xb key" (key -1: outside the map; only
// when the tables passed), per distance "slot k".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "liftmap.h"

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
    const int64_t n_scaf = next_ll(fh), n_seq = next_ll(fh), r = next_ll(fh);
    std::unique_ptr<int64_t[]> size(new int64_t[n_scaf]), off(new int64_t[n_scaf]), seq_size(new int64_t[n_seq]);
    std::unique_ptr<int32_t[]> seq(new int32_t[n_scaf]), first(new int32_t[n_seq]);
    std::unique_ptr<uint8_t[]> rev(new uint8_t[n_scaf]);
    for (int64_t s = 0; s < n_scaf; s++) {
        size[s] = next_ll(fh); seq[s] = (int32_t)next_ll(fh); off[s] = next_ll(fh); rev[s] = (uint8_t)next_ll(fh);
    }
    for (int64_t q = 0; q < n_seq; q++) seq_size[q] = next_ll(fh);
    char msg[256] = "";
    const int rc = lift_check_tables(size.get(), n_scaf, seq.get(), off.get(), rev.get(), seq_size.get(), n_seq, msg, sizeof(msg));
    printf("check %d %s\n", rc, msg);
    int64_t m = 0;
    if (!rc)
        for (int64_t q = 0; q < n_seq; q++) {
            first[q] = (int32_t)m;
            m += seq_size[q] / r + (seq_size[q] % r != 0);
        }
    LiftTables L;
    L.seq = seq.get(); L.off = off.get(); L.rev = rev.get(); L.scaf_size = size.get();
    L.n_scaf = (int32_t)n_scaf; L.n_seq = (int32_t)n_seq;
    expect(fh, 'P');
    const int64_t n_pairs = next_ll(fh);
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t sa = (int32_t)next_ll(fh); const int64_t pa = next_ll(fh);
        const int32_t sb = (int32_t)next_ll(fh); const int64_t pb = next_ll(fh);
        if (rc) continue;
        int32_t qa, qb;
        int64_t xa = 0, xb = 0;
        const bool ok_a = lift_end(L, sa, pa, &qa, &xa), ok_b = lift_end(L, sb, pb, &qb, &xb);
        long long key = -1;
        if (ok_a && ok_b) {
            const unsigned long long k = map_cell_key(qa, xa, qb, xb, first.get(), (int)n_seq, r, (int)m);
            if (k != kNoKey) key = (long long)k;
        }
        printf("pair %d %" PRId64 " %d %" PRId64 " %lld\n", qa, xa, qb, xb, key);
    }
    expect(fh, 'D');
    const int64_t n_d = next_ll(fh);
    for (int64_t k = 0; k < n_d; k++) {
        unsigned long long d;
        if (fscanf(fh, "%llu", &d) != 1) { fprintf(stderr, "short case file\n"); return 2; }
        printf("slot %d\n", lift_decay_slot((uint64_t)d));
    }
    fclose(fh);
    return 0;
}
