// links_host_check.cpp - the zone, key, kind, hash, capacity and row arithmetic of csrc/links.h as host code, for a build
// with -fsanitize=address,undefined (tests/test_links_cpu.py writes the case file and compares the output with
// tests/links_reference.py).  Every array is a heap block of exactly its size, so a read past a table is reported.
//
// Case file, blank-separated:  L n_scaf window | n_scaf sizes | C n | n x (n_kept n_scaf) | P n | n x (sa pa sb pb).
// Output: per capacity case "capacity <slots> <bits>", per pair "pair <kind> <key> <slot at 10 bits> <slot at 31 bits>"
// (key 0 and slots 0 for a pair that is nowhere), "counters <linked> <middle>", "rows <n>" and per row
// "row <lo> <hi> <LL> <LR> <RL> <RR> <OTHER>": the keys counted in a find-or-insert table of links_capacity slots with the
// probe sequence the kernels use, its used slots sorted by links_sort_records and merged by links_merge_rows.
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
    const int64_t n_scaf = next_ll(fh), window = next_ll(fh);
    std::unique_ptr<int64_t[]> size(new int64_t[n_scaf]);
    for (int64_t s = 0; s < n_scaf; s++) size[s] = next_ll(fh);
    expect(fh, 'C');
    const int64_t n_cap = next_ll(fh);
    for (int64_t k = 0; k < n_cap; k++) {
        const int64_t kept = next_ll(fh), scaf = next_ll(fh);
        int bits = 0;
        const int64_t cap = links_capacity(kept, scaf, &bits);
        printf("capacity %" PRId64 " %d\n", cap, bits);
    }
    expect(fh, 'P');
    const int64_t n_pairs = next_ll(fh);
    int bits = 0;
    const int64_t cap = links_capacity(n_pairs, n_scaf, &bits);
    if (cap > LINKS_MAX_SLOTS) { fprintf(stderr, "a table of %" PRId64 " slots\n", cap); return 3; }
    std::unique_ptr<uint64_t[]> keys(new uint64_t[cap]), counts(new uint64_t[cap]());
    for (int64_t h = 0; h < cap; h++) keys[h] = LINKS_EMPTY;
    unsigned long long counters[LINKS_COUNTERS] = {0, 0};
    int64_t used = 0;
    for (int64_t p = 0; p < n_pairs; p++) {
        const int32_t sa = (int32_t)next_ll(fh); const int64_t pa = next_ll(fh);
        const int32_t sb = (int32_t)next_ll(fh); const int64_t pb = next_ll(fh);
        uint64_t key = 0;
        const int kind = links_classify(size.get(), n_scaf, sa, pa, sb, pb, window, &key);
        if (kind == LINKS_NOWHERE) { printf("pair %d 0 0 0\n", kind); continue; }
        counters[kind]++;
        printf("pair %d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", kind, key, links_slot(key, 10), links_slot(key, 31));
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
    printf("counters %llu %llu\n", counters[LINKS_LINKED], counters[LINKS_MIDDLE]);
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
