// k_ends.hip - read-pair links between the ends of ordered scaffolds (hicmi_ends_*).
//
// The placed scaffolds are ranked in the order they lie (ends.h).  A pair whose ends lie on two scaffolds of one sequence,
// at most `reach` ranks apart and both inside an end zone of `window` bases, adds 1 to one of the four counters
// (zone of the lower rank) x (zone of the higher rank) of the entry (lower rank, rank difference) of a table of unsigned
// 64-bit integers.  Integer adds commute: every kernel form, chunking and arrival order gives the same bits.
//   k_ends_count<true>   HICMI_ENDS_PLAIN=1: one thread per pair, one global 64-bit atomic add per linked pair.
//   k_ends_count<false>  the combining form, after k_span_mark: a 256-lane workgroup takes a slice of ENDS_SLICE pairs and
//                        sums equal counter indices in an open-addressing table in LDS (ENDS_SLOTS slots of a 4-byte key
//                        and a 4-byte count).  A pair that finds neither its index nor a free slot within ENDS_PROBES
//                        probes adds to global memory directly.  Then every used slot issues one global atomic add.  A
//                        sorted pair file sends a slice to a handful of counters.
//                        Both forms count the six kinds of pairs per wave (a ballot per kind), per workgroup in LDS, and
//                        add six numbers per workgroup to the global counters.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((ENDS_SLOTS & (ENDS_SLOTS - 1)) == 0 && ENDS_SLOTS == 1 << ENDS_SLOT_BITS, "the table is a power of two");
static_assert(ENDS_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");
static_assert(ENDS_PROBES >= 1 && ENDS_PROBES <= ENDS_SLOTS, "a probe sequence does not lap the table");
static_assert(ENDS_MAX_TABLE <= (int64_t)1 << 31, "a counter index is a 32-bit key of the table");

constexpr unsigned int kNoIndex = ~0u;

// one pair at the counter `index`: into the table, or directly when the table has no room within ENDS_PROBES probes
__device__ __forceinline__ void ends_add_lds(unsigned int* s_key, unsigned int* s_cnt, unsigned long long* __restrict__ table,
                                             unsigned int index)
{
    unsigned int h = (index * 0x9E3779B9u) >> (32 - ENDS_SLOT_BITS);
    for (int probe = 0; probe < ENDS_PROBES; probe++) {
        const unsigned int seen = atomicCAS(&s_key[h], kNoIndex, index);
        if (seen == kNoIndex || seen == index) { atomicAdd(&s_cnt[h], 1u); return; }
        h = (h + 1) & (ENDS_SLOTS - 1);
    }
    atomicAdd(table + index, 1ull);
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void k_ends_count(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                    const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                    int64_t n, LiftTables L, EndsGrid G, int64_t n_table,
                                                    unsigned long long* __restrict__ table, unsigned long long* __restrict__ counters)
{
    __shared__ unsigned int s_key[PLAIN ? 1 : ENDS_SLOTS];
    __shared__ unsigned int s_cnt[PLAIN ? 1 : ENDS_SLOTS];
    __shared__ unsigned int s_kind[ENDS_COUNTERS];
    const int t = threadIdx.x;
    if (!PLAIN)
        for (int s = t; s < ENDS_SLOTS; s += 256) { s_key[s] = kNoIndex; s_cnt[s] = 0u; }
    if (t < ENDS_COUNTERS) s_kind[t] = 0u;
    __syncthreads();
    constexpr int kPerLane = PLAIN ? 1 : ENDS_SLICE / 256;
    const int64_t base = (int64_t)blockIdx.x * (256 * kPerLane);
    for (int u = 0; u < kPerLane; u++) {
        const int64_t p = base + u * 256 + t;
        int kind = ENDS_NOWHERE;
        int64_t index = 0;
        if (p < n) kind = ends_classify(L, G, scaf_a[p], pos_a[p], scaf_b[p], pos_b[p], &index);
        if (kind == ENDS_LINKED && (index < 0 || index >= n_table)) kind = ENDS_NOWHERE;     // never outside the table
        if (kind == ENDS_LINKED) {
            if (PLAIN) atomicAdd(table + index, 1ull);
            else ends_add_lds(s_key, s_cnt, table, (unsigned int)index);
        }
        // the six counters: one ballot per kind and wave (every lane of the wave is here: no lane left the loop)
#pragma unroll
        for (int k = 0; k < ENDS_COUNTERS; k++) {
            const unsigned long long who = __ballot(kind == k);
            if ((t & 63) == 0 && who) atomicAdd(&s_kind[k], (unsigned int)__popcll(who));
        }
    }
    __syncthreads();
    if (!PLAIN)
        for (int s = t; s < ENDS_SLOTS; s += 256) {
            const unsigned int index = s_key[s];
            if (index != kNoIndex) atomicAdd(table + index, (unsigned long long)s_cnt[s]);
        }
    if (t < ENDS_COUNTERS && s_kind[t]) atomicAdd(counters + t, (unsigned long long)s_kind[t]);
}

void launch_ends_count(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       const LiftTables& lift, const EndsGrid& grid, int64_t n_table, void* table, void* counters, bool plain,
                       hipStream_t s)
{
    if (n <= 0) return;
    unsigned long long* tb = reinterpret_cast<unsigned long long*>(table);
    unsigned long long* k = reinterpret_cast<unsigned long long*>(counters);
    if (plain)
        hipLaunchKernelGGL(k_ends_count<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n, lift,
                           grid, n_table, tb, k);
    else
        hipLaunchKernelGGL(k_ends_count<false>, dim3((unsigned)((n + ENDS_SLICE - 1) / ENDS_SLICE)), dim3(256), 0, s, scaf_a, pos_a,
                           scaf_b, pos_b, n, lift, grid, n_table, tb, k);
}

}  // namespace hicmi
