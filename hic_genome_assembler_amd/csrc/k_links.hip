// k_links.hip - the end-link graph of all scaffolds from the resident pair store (hicmi_links_resident).
//
// Every stored pair has a 64-bit key (links.h): the two scaffolds in index order and the combination of the end zones its
// ends fall in.  The keys of a call are counted in a find-or-insert table in device memory: open addressing with linear
// probing, a key array that starts out as LINKS_EMPTY and a count array that starts out as 0, of a power-of-two capacity the
// host sizes so that the table is never more than half full.  A key is claimed by a 64-bit atomicCAS against LINKS_EMPTY and
// never changes afterwards, so no thread waits on another; every probe loop is bounded (the capacity here, LINKS_PROBES in
// LDS), and an insert that runs out of probes raises a flag the host turns into an error.  Integer adds commute: every
// kernel form, store order and mate order gives the same counts per key; the slot a key lands in depends on the race.
//   k_links_count<true>    HICMI_LINKS_PLAIN=1: one thread per pair, one find-or-insert and one 64-bit atomic add per pair.
//   k_links_count<false>   the combining form, after k_seats_count: a 256-lane workgroup takes a slice of LINKS_SLICE pairs
//                          and sums equal keys in an open-addressing table in LDS (LINKS_SLOTS slots of an 8-byte key and
//                          a 4-byte count).  An add that finds neither its key nor a free slot within LINKS_PROBES probes
//                          goes to the global table directly.  Then every used slot issues one global find-or-insert and add.
//                          Both forms count the two kinds of pairs per wave (a ballot per kind), per workgroup in LDS, and
//                          add two numbers per workgroup to the global counters.
//   k_links_count_lifted   the same two forms for hicmi_links_lifted: every end is lifted onto its sequence
//                          first - its scaffold's sequence, offset, reversal and size are gathered from the lift tables, then
//                          the size of its sequence - and the key is that of the two sequences (links_classify_lifted).  Four
//                          kinds of pairs, counted the same way: a ballot per kind and wave, four numbers per workgroup.
//   k_links_compact        the used slots into (key, count) records: a workgroup counts the used ones of LINKS_COMPACT_SLICE
//                          slots (a ballot per wave), bumps the record count once, and places them behind that (a ballot per
//                          wave, a cursor in LDS).  The order of the records is the race's; the host sorts them.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((LINKS_SLOTS & (LINKS_SLOTS - 1)) == 0 && LINKS_SLOTS == 1 << LINKS_SLOT_BITS, "the table is a power of two");
static_assert(LINKS_SLICE % 256 == 0 && LINKS_COMPACT_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");
static_assert(LINKS_PROBES >= 1 && LINKS_PROBES <= LINKS_SLOTS, "a probe sequence does not lap the table");
static_assert(LINKS_SLOTS * (sizeof(unsigned long long) + sizeof(unsigned int)) <= 64 * 1024, "key and count of every slot fit the LDS of a workgroup");
static_assert(LINKS_EXTRAS == LINKS_COUNTERS + 2, "the counters, the flag and the number of records");
static_assert(LINKS_LIFTED_LINKED == LINKS_LINKED && LINKS_LIFTED_MIDDLE == LINKS_MIDDLE && links_lifted_extra(LINKS_LIFTED_INSIDE) == LINKS_EXTRAS &&
              links_lifted_extra(LINKS_LIFTED_UNLIFTED) == LINKS_LIFTED_EXTRAS - 1, "the lifted count keeps the flag and the records where they are");

// `add` at `key` in the global table: the slot that holds the key, or the first free one of its probe sequence
__device__ __forceinline__ void links_add_global(const LinksTable& T, unsigned long long key, unsigned long long add)
{
    const unsigned long long mask = (unsigned long long)T.cap - 1ull;
    unsigned long long h = links_slot(key, T.bits) & mask;
    for (long long probe = 0; probe < T.cap; probe++) {
        const unsigned long long seen = atomicCAS(T.keys + h, (unsigned long long)LINKS_EMPTY, key);
        if (seen == LINKS_EMPTY || seen == key) { atomicAdd(T.counts + h, add); return; }
        h = (h + 1ull) & mask;
    }
    atomicOr(T.extras + LINKS_FLAG, 1ull);                         // a full table: the host refuses the result
}

// one pair at `key`: into the table in LDS, or into the global one when there is no room within LINKS_PROBES probes
__device__ __forceinline__ void links_add_lds(unsigned long long* s_key, unsigned int* s_cnt, const LinksTable& T, unsigned long long key)
{
    unsigned int h = (unsigned int)links_slot(key, LINKS_SLOT_BITS);
    for (int probe = 0; probe < LINKS_PROBES; probe++) {
        const unsigned long long seen = atomicCAS(&s_key[h], (unsigned long long)LINKS_EMPTY, key);
        if (seen == LINKS_EMPTY || seen == key) { atomicAdd(&s_cnt[h], 1u); return; }
        h = (h + 1u) & (LINKS_SLOTS - 1);
    }
    links_add_global(T, key, 1ull);
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void k_links_count(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                     const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b, int64_t n,
                                                     const int64_t* __restrict__ scaf_size, int64_t n_scaf, int64_t window, LinksTable T)
{
    __shared__ unsigned long long s_key[PLAIN ? 1 : LINKS_SLOTS];
    __shared__ unsigned int s_cnt[PLAIN ? 1 : LINKS_SLOTS];
    __shared__ unsigned int s_kind[LINKS_COUNTERS];
    const int t = threadIdx.x;
    if (!PLAIN)
        for (int s = t; s < LINKS_SLOTS; s += 256) { s_key[s] = LINKS_EMPTY; s_cnt[s] = 0u; }
    if (t < LINKS_COUNTERS) s_kind[t] = 0u;
    __syncthreads();
    constexpr int kPerLane = PLAIN ? 1 : LINKS_SLICE / 256;
    const int64_t base = (int64_t)blockIdx.x * (256 * kPerLane);
    for (int u = 0; u < kPerLane; u++) {
        const int64_t p = base + u * 256 + t;
        int kind = LINKS_NOWHERE;
        uint64_t key = LINKS_EMPTY;
        if (p < n) kind = links_classify(scaf_size, n_scaf, scaf_a[p], pos_a[p], scaf_b[p], pos_b[p], window, &key);
        if (kind != LINKS_NOWHERE) {
            if (PLAIN) links_add_global(T, (unsigned long long)key, 1ull);
            else links_add_lds(s_key, s_cnt, T, (unsigned long long)key);
        }
        // the two counters: one ballot per kind and wave (every lane of the wave is here: no lane left the loop)
#pragma unroll
        for (int k = 0; k < LINKS_COUNTERS; k++) {
            const unsigned long long who = __ballot(kind == k);
            if ((t & 63) == 0 && who) atomicAdd(&s_kind[k], (unsigned int)__popcll(who));
        }
    }
    __syncthreads();
    if (!PLAIN)
        for (int s = t; s < LINKS_SLOTS; s += 256) {
            const unsigned long long key = s_key[s];
            if (key != LINKS_EMPTY) links_add_global(T, key, (unsigned long long)s_cnt[s]);
        }
    if (t < LINKS_COUNTERS && s_kind[t]) atomicAdd(T.extras + t, (unsigned long long)s_kind[t]);
}

// The count on lifted ends.  The table in LDS, the probing and the spill are those of k_links_count; the lift tables and the
// sequence sizes are a few bytes per scaffold, read by every pair and so served from the caches.
template <bool PLAIN>
__global__ __launch_bounds__(256) void k_links_count_lifted(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                            const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b, int64_t n,
                                                            LiftTables L, const int64_t* __restrict__ seq_size, int64_t window, LinksTable T)
{
    __shared__ unsigned long long s_key[PLAIN ? 1 : LINKS_SLOTS];
    __shared__ unsigned int s_cnt[PLAIN ? 1 : LINKS_SLOTS];
    __shared__ unsigned int s_kind[LINKS_LIFTED_COUNTERS];
    const int t = threadIdx.x;
    if (!PLAIN)
        for (int s = t; s < LINKS_SLOTS; s += 256) { s_key[s] = LINKS_EMPTY; s_cnt[s] = 0u; }
    if (t < LINKS_LIFTED_COUNTERS) s_kind[t] = 0u;
    __syncthreads();
    constexpr int kPerLane = PLAIN ? 1 : LINKS_SLICE / 256;
    const int64_t base = (int64_t)blockIdx.x * (256 * kPerLane);
    for (int u = 0; u < kPerLane; u++) {
        const int64_t p = base + u * 256 + t;
        int kind = LINKS_LIFTED_NOWHERE;
        uint64_t key = LINKS_EMPTY;
        if (p < n) kind = links_classify_lifted(L, seq_size, scaf_a[p], pos_a[p], scaf_b[p], pos_b[p], window, &key);
        if (kind == LINKS_LIFTED_LINKED || kind == LINKS_LIFTED_MIDDLE) {
            if (PLAIN) links_add_global(T, (unsigned long long)key, 1ull);
            else links_add_lds(s_key, s_cnt, T, (unsigned long long)key);
        }
        // the four counters: one ballot per kind and wave (every lane of the wave is here: no lane left the loop)
#pragma unroll
        for (int k = 0; k < LINKS_LIFTED_COUNTERS; k++) {
            const unsigned long long who = __ballot(kind == k);
            if ((t & 63) == 0 && who) atomicAdd(&s_kind[k], (unsigned int)__popcll(who));
        }
    }
    __syncthreads();
    if (!PLAIN)
        for (int s = t; s < LINKS_SLOTS; s += 256) {
            const unsigned long long key = s_key[s];
            if (key != LINKS_EMPTY) links_add_global(T, key, (unsigned long long)s_cnt[s]);
        }
    if (t < LINKS_LIFTED_COUNTERS && s_kind[t]) atomicAdd(T.extras + links_lifted_extra(t), (unsigned long long)s_kind[t]);
}

// the used slots as records; a record that finds no room (the host sized rec_cap for every key a call can see) raises the flag.
// Two passes over the workgroup's LINKS_COMPACT_SLICE slots: the first counts the used ones, the second places them.
__global__ __launch_bounds__(256) void k_links_compact(LinksTable T, unsigned long long* __restrict__ rec_key,
                                                       unsigned long long* __restrict__ rec_cnt, int64_t rec_cap)
{
    __shared__ unsigned int s_used, s_cursor;
    __shared__ unsigned long long s_first;
    const int t = threadIdx.x, lane = t & 63;
    if (t == 0) { s_used = 0u; s_cursor = 0u; }
    __syncthreads();
    constexpr int kPerLane = LINKS_COMPACT_SLICE / 256;
    const int64_t base = (int64_t)blockIdx.x * LINKS_COMPACT_SLICE;
    for (int u = 0; u < kPerLane; u++) {
        const int64_t s = base + u * 256 + t;
        const unsigned long long who = __ballot(s < T.cap && T.keys[s] != LINKS_EMPTY);   // every lane of the wave is here
        if (lane == 0 && who) atomicAdd(&s_used, (unsigned int)__popcll(who));
    }
    __syncthreads();
    if (t == 0 && s_used) s_first = atomicAdd(T.extras + LINKS_RECORDS, (unsigned long long)s_used);
    __syncthreads();
    if (!s_used) return;                                           // the whole workgroup leaves together
    const unsigned long long first = s_first;
    for (int u = 0; u < kPerLane; u++) {
        const int64_t s = base + u * 256 + t;
        unsigned long long key = LINKS_EMPTY;
        if (s < T.cap) key = T.keys[s];
        const bool used = key != LINKS_EMPTY;
        const unsigned long long who = __ballot(used);
        unsigned int wave_at = 0u;
        if (lane == 0 && who) wave_at = atomicAdd(&s_cursor, (unsigned int)__popcll(who));
        wave_at = __shfl(wave_at, 0);
        if (!used) continue;
        const unsigned long long at = first + wave_at + (unsigned long long)__popcll(who & ((1ull << lane) - 1ull));
        if (at >= (unsigned long long)rec_cap) { atomicOr(T.extras + LINKS_FLAG, 2ull); continue; }   // never outside the records
        rec_key[at] = key;
        rec_cnt[at] = T.counts[s];
    }
}

void launch_links_count(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                        const int64_t* scaf_size, int64_t n_scaf, int64_t window, const LinksTable& table, bool plain, hipStream_t s)
{
    if (n <= 0) return;
    if (plain)
        hipLaunchKernelGGL((k_links_count<true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n,
                           scaf_size, n_scaf, window, table);
    else
        hipLaunchKernelGGL((k_links_count<false>), dim3((unsigned)((n + LINKS_SLICE - 1) / LINKS_SLICE)), dim3(256), 0, s, scaf_a, pos_a,
                           scaf_b, pos_b, n, scaf_size, n_scaf, window, table);
}

void launch_links_count_lifted(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                               const LiftTables& lift, const int64_t* seq_size, int64_t window, const LinksTable& table, bool plain,
                               hipStream_t s)
{
    if (n <= 0) return;
    if (plain)
        hipLaunchKernelGGL((k_links_count_lifted<true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b,
                           n, lift, seq_size, window, table);
    else
        hipLaunchKernelGGL((k_links_count_lifted<false>), dim3((unsigned)((n + LINKS_SLICE - 1) / LINKS_SLICE)), dim3(256), 0, s, scaf_a,
                           pos_a, scaf_b, pos_b, n, lift, seq_size, window, table);
}

void launch_links_compact(const LinksTable& table, void* rec_key, void* rec_cnt, int64_t rec_cap, hipStream_t s)
{
    hipLaunchKernelGGL(k_links_compact, dim3((unsigned)((table.cap + LINKS_COMPACT_SLICE - 1) / LINKS_COMPACT_SLICE)), dim3(256), 0, s, table,
                       reinterpret_cast<unsigned long long*>(rec_key), reinterpret_cast<unsigned long long*>(rec_cnt), rec_cap);
}

}  // namespace hicmi
