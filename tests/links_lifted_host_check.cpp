// links_lifted_host_check.cpp - links_classify_lifted of csrc/links.h as host code, for a build with
// -fsanitize=address,undefined (tests/test_links_lifted_cpu.py writes the case file and compares the output with
// tests/links_lifted_reference.py).  Every array is a heap block of exactly its size, so a read past a table is reported.
//
// Case file, blank-separated:  L n_scaf n_seq window | n_scaf sizes | n_scaf lift_seq | n_scaf lift_off | n_scaf lift_rev |
// n_seq seq_sizes | P n | n x (sa pa sb pb).
// Output: per pair "pair <kind> <key>" (key 0 for a pair without one), "counters <linked> <middle> <inside> <unlifted>",
// "rows <n>" and per row "row <lo> <hi> <LL> <LR> <RL> <RR> <OTHER>": the keys counted in a find-or-insert table of
// links_capacity(pairs, n_seq) slots with the probe sequence the kernels use, sorted and merged as the library does.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "links.h"

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
    expect(fh, 'L');
    const int64_t n_scaf = next_ll(fh), n_seq = next_ll(fh), window = next_ll(fh);
    std::unique_ptr<int64_t[]> size(new int64_t[n_scaf]), off(new int64_t[n_scaf]), seq_size(new int64_t[n_seq]);
    std::unique_ptr<int32_t[]> seq(new int32_t[n_scaf]);
    std::unique_ptr<uint8_t[]> rev(new uint8_t[n_scaf]);
    for (int64_t s = 0; s < n_scaf; s++) size[s] = next_ll(fh);
    for (int64_t s = 0; s < n_scaf; s++) seq[s] = (int32_t)next_ll(fh);
    for (int64_t s = 0; s < n_scaf; s++) off[s] = next_ll(fh);
    for (int64_t s = 0; s < n_scaf; s++) rev[s] = (uint8_t)next_ll(fh);
    for (int64_t q = 0; q < n_seq; q++) seq_size[q] = next_ll(fh);
    char msg[256];
    if (lift_check_tables(size.get(), n_scaf, seq.get(), off.get(), rev.get(), seq_size.get(), n_seq, msg, sizeof(msg))) {
        fprintf(stderr, "the tables are refused: %s\n", msg);
        return 3;
    }
    LiftTables L;
    L.seq = seq.get(); L.off = off.get(); L.rev = rev.get(); L.scaf_size = size.get();
    L.n_scaf = (int32_t)n_scaf; L.n_seq = (int32_t)n_seq;
    expect(fh, 'P');
    const int64_t n_pairs = next_ll(fh);
    int bits = 0;
    const int64_t cap = links_capacity(n_pairs, n_seq, &bits);
    if (cap > LINKS_MAX_SLOTS) { fprintf(stderr, "a table of %" PRId64 " slots\n", cap); return 3; }
    std::unique_ptr<uint64_t[]> keys(new uint64_t[cap]), counts(new uint64_t[cap]());
    for (int64_t h = 0; h < cap; h++) keys[h] = LINKS_EMPTY;
    unsigned long long counters[LINKS_LIFTED_COUNTERS] = {0, 0, 0, 0};
    int64_t used = 0;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t sa = (int32_t)next_ll(fh); const int64_t pa = next_ll(fh);
        const int32_t sb = (int32_t)next_ll(fh); const int64_t pb = next_ll(fh);
        uint64_t key = 0;
        const int kind = links_classify_lifted(L, seq_size.get(), sa, pa, sb, pb, window, &key);
        if (kind == LINKS_LIFTED_NOWHERE) { printf("pair %d 0\n", kind); continue; }
        counters[kind]++;
        if (kind != LINKS_LIFTED_LINKED && kind != LINKS_LIFTED_MIDDLE) { printf("pair %d 0\n", kind); continue; }
        printf("pair %d %" PRIu64 "\n", kind, key);
        if (key == LINKS_EMPTY) { fprintf(stderr, "pair %" PRId64 ": the key is the empty mark\n", p); return 3; }
        uint64_t h = links_slot(key, bits);
        int64_t probe = 0;
        for (; probe < cap; probe++) {
            if (h >= (uint64_t)cap) { fprintf(stderr, "pair %" PRId64 ": slot %" PRIu64 " outside the table\n", p, h); return 3; }
            if (keys[h] == LINKS_EMPTY) { keys[h] = key; used++; }
            if (keys[h] == key) { counts[h]++; break; }
            h = (h + 1) & (uint64_t)(cap - 1);
        }
        if (probe == cap) { fprintf(stderr, "pair %" PRId64 ": the table is full\n", p); return 3; }
        if (2 * used > cap) { fprintf(stderr, "pair %" PRId64 ": the table is more than half full\n", p); return 3; }
    }
    printf("counters %llu %llu %llu %llu\n", counters[LINKS_LIFTED_LINKED], counters[LINKS_LIFTED_MIDDLE], counters[LINKS_LIFTED_INSIDE],
           counters[LINKS_LIFTED_UNLIFTED]);
    std::unique_ptr<uint64_t[]> rec_key(new uint64_t[used]), rec_cnt(new uint64_t[used]), counts5(new uint64_t[used * LINKS_COMBOS]);
    std::unique_ptr<int32_t[]> lo(new int32_t[used]), hi(new int32_t[used]);
    int64_t n_rec = 0;
    for (int64_t h = 0; h < cap; h++)                             // in slot order, as the device compacts them
        if (keys[h] != LINKS_EMPTY) { rec_key[n_rec] = keys[h]; rec_cnt[n_rec] = counts[h]; n_rec++; }
    links_sort_records(rec_key.get(), rec_cnt.get(), n_rec);
    const int64_t n_rows = links_merge_rows(rec_key.get(), rec_cnt.get(), n_rec, lo.get(), hi.get(), counts5.get());
    printf("rows %" PRId64 "\n", n_rows);
    for (int64_t r = 0; r < n_rows; r++) {
        printf("row %d %d", lo[r], hi[r]);
        for (int k = 0; k < LINKS_COMBOS; k++) printf(" %" PRIu64, counts5[r * LINKS_COMBOS + k]);
        printf("\n");
    }
    fclose(fh);
    return 0;
}
