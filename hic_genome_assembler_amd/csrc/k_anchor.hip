// k_anchor.hip - read-pair links between the scaffolds an ordering leaves out and the placed ones (hicmi_anchor_*;
// DESIGN.md 9q).
//
// A candidate - a dropped scaffold of size > 0 - owns a block of counters of a table of unsigned 64-bit integers
// (anchor.h): one per sequence in sequence mode, and in rank mode four - (half of the candidate) x (end zone of the placed
// scaffold) - per placed scaffold of its target sequence.  A pair with one end on a candidate and the other on a placed
// scaffold adds 1 to one counter.  Integer adds commute: every kernel form, chunking and arrival order gives the same bits.
//   k_anchor_count<RANK_MODE, true>   HICMI_ANCHOR_PLAIN=1: one thread per pair, one global 64-bit atomic add per anchored
//                                     pair.
//   k_anchor_count<RANK_MODE, false>  the combining form, after k_ends_count: a 256-lane workgroup takes a slice of
//                                     ANCHOR_SLICE pairs and sums equal counter indices in an open-addressing table in LDS
//                                     (ANCHOR_SLOTS slots of a 4-byte key and a 4-byte count).  A pair that finds neither
//                                     its index nor a free slot within ANCHOR_PROBES probes adds to global memory
//                                     directly.  Then every used slot issues one global atomic add.
//                                     Both forms count the six kinds of pairs per wave (a ballot per kind), per workgroup
//                                     in LDS, and add six numbers per workgroup to the global counters.
// A merge of equal indices inside the wave before the table (a ballot per distinct index, the first lane adding the
// popcount) was measured and left out: it is slower in sequence mode and no faster in rank mode.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((ANCHOR_SLOTS & (ANCHOR_SLOTS - 1)) == 0 && ANCHOR_SLOTS == 1 << ANCHOR_SLOT_BITS, "the table is a power of two");
static_assert(ANCHOR_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");
static_assert(ANCHOR_PROBES >= 1 && ANCHOR_PROBES <= ANCHOR_SLOTS, "a probe sequence does not lap the table");
static_assert(ANCHOR_MAX_TABLE <= (int64_t)1 << 31, "a counter index is a 32-bit key of the table");

constexpr unsigned int kNoAnchor = ~0u;

// one pair at the counter `index`: into the table, or directly when the table has no room within ANCHOR_PROBES probes
__device__ __forceinline__ void anchor_add_lds(unsigned int* s_key, unsigned int* s_cnt, unsigned long long* __restrict__ table,
                                               unsigned int index)
{
    unsigned int h = (index * 0x9E3779B9u) >> (32 - ANCHOR_SLOT_BITS);
    for (int probe = 0; probe < ANCHOR_PROBES; probe++) {
        const unsigned int seen = atomicCAS(&s_key[h], kNoAnchor, index);
        if (seen == kNoAnchor || seen == index) { atomicAdd(&s_cnt[h], 1u); return; }
        h = (h + 1) & (ANCHOR_SLOTS - 1);
    }
    atomicAdd(table + index, 1ull);
}

template <bool RANK_MODE, bool PLAIN>
__global__ __launch_bounds__(256) void k_anchor_count(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                      const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                      int64_t n, LiftTables L, AnchorGrid G, int64_t n_table,
                                                      unsigned long long* __restrict__ table, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned int s_key[PLAIN ? 1 : ANCHOR_SLOTS];
    __shared__ unsigned int s_cnt[PLAIN ? 1 : ANCHOR_SLOTS];
    __shared__ unsigned int s_kind[ANCHOR_COUNTERS];
    const int t = threadIdx.x;
    if (!PLAIN)
        for (int s = t; s < ANCHOR_SLOTS; s += 256) { s_key[s] = kNoAnchor; s_cnt[s] = 0u; }
    if (t < ANCHOR_COUNTERS) s_kind[t] = 0u;
    __syncthreads();
    constexpr int kPerLane = PLAIN ? 1 : ANCHOR_SLICE / 256;
    const int64_t base = (int64_t)blockIdx.x * (256 * kPerLane);
    for (int u = 0; u < kPerLane; u++) {
        const int64_t p = base + u * 256 + t;
        int kind = ANCHOR_NOWHERE;
        int64_t index = 0;
        if (p < n) kind = anchor_classify<RANK_MODE>(L, G, scaf_a[p], pos_a[p], scaf_b[p], pos_b[p], &index);
        if (kind == ANCHOR_ANCHORED && (index < 0 || index >= n_table)) kind = ANCHOR_NOWHERE;     // never outside the table
        if (kind == ANCHOR_ANCHORED) {
            if (PLAIN) atomicAdd(table + index, 1ull);
            else anchor_add_lds(s_key, s_cnt, table, (unsigned int)index);
        }
        // the six counters: one ballot per kind and wave (every lane of the wave is here: no lane left the loop)
#pragma unroll
        for (int k = 0; k < ANCHOR_COUNTERS; k++) {
            const unsigned long long who = __ballot(kind == k);
            if ((t & 63) == 0 && who) atomicAdd(&s_kind[k], (unsigned int)__popcll(who));
        }
    }
    __syncthreads();
    if (!PLAIN)
        for (int s = t; s < ANCHOR_SLOTS; s += 256) {
            const unsigned int index = s_key[s];
            if (index != kNoAnchor) atomicAdd(table + index, (unsigned long long)s_cnt[s]);
        }
    if (t < ANCHOR_COUNTERS && s_kind[t]) atomicAdd(counters + t, (unsigned long long)s_kind[t]);
}

template <bool RANK_MODE>
static void launch_anchor_mode(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                               const LiftTables& lift, const AnchorGrid& grid, int64_t n_table, unsigned long long* tb,
                               unsigned long long* k, bool plain, hipStream_t s)
{
    if (plain)
        hipLaunchKernelGGL((k_anchor_count<RANK_MODE, true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b,
                           pos_b, n, lift, grid, n_table, tb, k);
    else
        hipLaunchKernelGGL((k_anchor_count<RANK_MODE, false>), dim3((unsigned)((n + ANCHOR_SLICE - 1) / ANCHOR_SLICE)), dim3(256), 0, s,
                           scaf_a, pos_a, scaf_b, pos_b, n, lift, grid, n_table, tb, k);
}

void launch_anchor_count(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                         const LiftTables& lift, const AnchorGrid& grid, int64_t n_table, void* table, void* counters, bool plain,
                         hipStream_t s)
{
    if (n <= 0) return;
    unsigned long long* tb = reinterpret_cast<unsigned long long*>(table);
    unsigned long long* k = reinterpret_cast<unsigned long long*>(counters);
    if (grid.target) launch_anchor_mode<true>(scaf_a, pos_a, scaf_b, pos_b, n, lift, grid, n_table, tb, k, plain, s);
    else launch_anchor_mode<false>(scaf_a, pos_a, scaf_b, pos_b, n, lift, grid, n_table, tb, k, plain, s);
}

}  // namespace hicmi
