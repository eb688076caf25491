// k_seats.hip - read-pair links of every placed scaffold with the chromosomes and with the end zones of the scaffolds of its
// own chromosome (hicmi_seats_resident).
//
// A placed scaffold with a base owns a block of counters of a table of unsigned 64-bit integers (seats.h): one per sequence
// and four - (half of the scaffold) x (end zone of the other scaffold) - per placed scaffold of its own sequence.  A pair
// between two placed scaffolds adds 1 to two chromosome counters and, inside one sequence, to up to two gap counters: it is
// evidence about the seat of both.  Integer adds commute: every kernel form, store order and mate order gives the same bits.
//   k_seats_count<true>    HICMI_SEATS_PLAIN=1: one thread per pair, up to four global 64-bit atomic adds per pair.
//   k_seats_count<false>   the combining form, after k_anchor_count: a 256-lane workgroup takes a slice of SEATS_SLICE pairs
//                          and sums equal counter indices in an open-addressing table in LDS (SEATS_SLOTS slots of a 4-byte
//                          key and a 4-byte count).  An add that finds neither its index nor a free slot within SEATS_PROBES
//                          probes goes to global memory directly.  Then every used slot issues one global atomic add.
//                          Both forms count the five kinds of pairs per wave (a ballot per kind), per workgroup in LDS, and
//                          add five numbers per workgroup to the global counters.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((SEATS_SLOTS & (SEATS_SLOTS - 1)) == 0 && SEATS_SLOTS == 1 << SEATS_SLOT_BITS, "the table is a power of two");
static_assert(SEATS_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");
static_assert(SEATS_PROBES >= 1 && SEATS_PROBES <= SEATS_SLOTS, "a probe sequence does not lap the table");
static_assert(SEATS_MAX_TABLE <= (int64_t)1 << 31, "a counter index is a 32-bit key of the table");
static_assert(2 * SEATS_SLOTS * sizeof(unsigned int) <= 64 * 1024, "key and count of every slot fit the LDS of a workgroup");

constexpr unsigned int kNoSeat = ~0u;

// one add at the counter `index`: into the table, or directly when the table has no room within SEATS_PROBES probes
__device__ __forceinline__ void seats_add_lds(unsigned int* s_key, unsigned int* s_cnt, unsigned long long* __restrict__ table,
                                              unsigned int index)
{
    unsigned int h = (index * 0x9E3779B9u) >> (32 - SEATS_SLOT_BITS);
    for (int probe = 0; probe < SEATS_PROBES; probe++) {
        const unsigned int seen = atomicCAS(&s_key[h], kNoSeat, index);
        if (seen == kNoSeat || seen == index) { atomicAdd(&s_cnt[h], 1u); return; }
        h = (h + 1) & (SEATS_SLOTS - 1);
    }
    atomicAdd(table + index, 1ull);
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void k_seats_count(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                     const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b, int64_t n,
                                                     LiftTables L, SeatsGrid G, int64_t n_table, unsigned long long* __restrict__ table,
                                                     unsigned long long* __restrict__ counters)
{
    __shared__ unsigned int s_key[PLAIN ? 1 : SEATS_SLOTS];
    __shared__ unsigned int s_cnt[PLAIN ? 1 : SEATS_SLOTS];
    __shared__ unsigned int s_kind[SEATS_COUNTERS];
    const int t = threadIdx.x;
    if (!PLAIN)
        for (int s = t; s < SEATS_SLOTS; s += 256) { s_key[s] = kNoSeat; s_cnt[s] = 0u; }
    if (t < SEATS_COUNTERS) s_kind[t] = 0u;
    __syncthreads();
    constexpr int kPerLane = PLAIN ? 1 : SEATS_SLICE / 256;
    const int64_t base = (int64_t)blockIdx.x * (256 * kPerLane);
    for (int u = 0; u < kPerLane; u++) {
        const int64_t p = base + u * 256 + t;
        int kind = SEATS_NOWHERE, n_index = 0;
        int64_t index[4] = {0, 0, 0, 0};
        if (p < n) kind = seats_classify(L, G, scaf_a[p], pos_a[p], scaf_b[p], pos_b[p], index, &n_index);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n_index && (index[k] < 0 || index[k] >= n_table)) kind = SEATS_NOWHERE;     // never outside the table
        if (kind == SEATS_NOWHERE) n_index = 0;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (k < n_index) {
                if (PLAIN) atomicAdd(table + index[k], 1ull);
                else seats_add_lds(s_key, s_cnt, table, (unsigned int)index[k]);
            }
        // the five counters: one ballot per kind and wave (every lane of the wave is here: no lane left the loop)
#pragma unroll
        for (int k = 0; k < SEATS_COUNTERS; k++) {
            const unsigned long long who = __ballot(kind == k);
            if ((t & 63) == 0 && who) atomicAdd(&s_kind[k], (unsigned int)__popcll(who));
        }
    }
    __syncthreads();
    if (!PLAIN)
        for (int s = t; s < SEATS_SLOTS; s += 256) {
            const unsigned int index = s_key[s];
            if (index != kNoSeat) atomicAdd(table + index, (unsigned long long)s_cnt[s]);
        }
    if (t < SEATS_COUNTERS && s_kind[t]) atomicAdd(counters + t, (unsigned long long)s_kind[t]);
}

void launch_seats_count(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                        const LiftTables& lift, const SeatsGrid& grid, int64_t n_table, void* table, void* counters, bool plain,
                        hipStream_t s)
{
    if (n <= 0) return;
    unsigned long long* tb = reinterpret_cast<unsigned long long*>(table);
    unsigned long long* k = reinterpret_cast<unsigned long long*>(counters);
    if (plain)
        hipLaunchKernelGGL((k_seats_count<true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n, lift,
                           grid, n_table, tb, k);
    else
        hipLaunchKernelGGL((k_seats_count<false>), dim3((unsigned)((n + SEATS_SLICE - 1) / SEATS_SLICE)), dim3(256), 0, s, scaf_a, pos_a,
                           scaf_b, pos_b, n, lift, grid, n_table, tb, k);
}

}  // namespace hicmi
