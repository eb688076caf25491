// k_pairs.hip - the resident pair store (hicmi_pairs_*).
//
// A chunk of pairs on the device is compacted into the store: a pair whose ends lie on two scaffolds is kept (pairs.h) and
// appended at the store's end, a pair on one scaffold s adds 1 to intra[s].  The store's length lives on the device.
//   k_pairs_keep<true>    HICMI_PAIRS_PLAIN=1: one thread per pair, one atomic bump of the length per kept pair, one global
//                         atomic add per intra pair.  The store is the same multiset in an order that changes from run to run.
//   k_pairs_keep<false>   the stable form, three launches after k_span_scan.  k_pairs_count: a 256-lane workgroup takes a
//                         slice of PAIRS_SLICE pairs, counts its kept pairs (a ballot and a popcount per wave) and sums the
//                         intra pairs per scaffold in an open-addressing table in LDS (PAIRS_SLOTS slots of a 4-byte key
//                         and a 4-byte count; a pair that finds no room within PAIRS_PROBES probes adds to global memory
//                         directly), so that a sorted file sends one add per slice and scaffold to global memory.
//                         k_pairs_scan: one workgroup turns the counts of all workgroups into the places their kept pairs
//                         start at, from the length on, and advances the length.  k_pairs_keep<false>: every workgroup
//                         takes its slice again, numbers its kept pairs in the order they come (ballot, popcount of the
//                         lanes below, the counts of the waves before) and writes them.  The store is the boolean mask of
//                         the input.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((PAIRS_SLOTS & (PAIRS_SLOTS - 1)) == 0 && PAIRS_SLOTS == 1 << PAIRS_SLOT_BITS, "the table is a power of two");
static_assert(PAIRS_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");
static_assert(PAIRS_PROBES >= 1 && PAIRS_PROBES <= PAIRS_SLOTS, "a probe sequence does not lap the table");

constexpr unsigned int kNoScaffold = ~0u;
constexpr int kRounds = PAIRS_SLICE / 256;     // rounds of 256 consecutive pairs of a slice
constexpr int kParts = kRounds * 4;            // (round, wave): 64 consecutive pairs each

// one intra pair on scaffold s: into the table, or directly when the table has no room within PAIRS_PROBES probes
__device__ __forceinline__ void pairs_intra_lds(unsigned int* s_key, unsigned int* s_cnt, unsigned long long* __restrict__ intra,
                                                unsigned int s)
{
    unsigned int h = (s * 0x9E3779B9u) >> (32 - PAIRS_SLOT_BITS);
    for (int probe = 0; probe < PAIRS_PROBES; probe++) {
        const unsigned int seen = atomicCAS(&s_key[h], kNoScaffold, s);
        if (seen == kNoScaffold || seen == s) { atomicAdd(&s_cnt[h], 1u); return; }
        h = (h + 1) & (PAIRS_SLOTS - 1);
    }
    atomicAdd(intra + s, 1ull);
}

__global__ __launch_bounds__(256) void k_pairs_count(const int32_t* __restrict__ scaf_a, const int32_t* __restrict__ scaf_b, int64_t n,
                                                     int64_t n_scaf, unsigned long long* __restrict__ intra,
                                                     long long* __restrict__ block_kept)
{
    __shared__ unsigned int s_key[PAIRS_SLOTS];
    __shared__ unsigned int s_cnt[PAIRS_SLOTS];
    __shared__ unsigned int s_kept;
    const int t = threadIdx.x;
    for (int s = t; s < PAIRS_SLOTS; s += 256) { s_key[s] = kNoScaffold; s_cnt[s] = 0u; }
    if (t == 0) s_kept = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * PAIRS_SLICE;
    for (int u = 0; u < kRounds; u++) {
        const int64_t p = base + u * 256 + t;
        bool kept = false;
        if (p < n) {
            const int32_t sa = scaf_a[p];
            kept = pairs_kept(sa, scaf_b[p]);
            if (!kept && sa >= 0 && sa < n_scaf) pairs_intra_lds(s_key, s_cnt, intra, (unsigned int)sa);   // never outside intra[]
        }
        const unsigned long long who = __ballot(kept);            // every lane of the wave is here: no lane left the loop
        if ((t & 63) == 0 && who) atomicAdd(&s_kept, (unsigned int)__popcll(who));
    }
    __syncthreads();
    for (int s = t; s < PAIRS_SLOTS; s += 256) {
        const unsigned int scaffold = s_key[s];
        if (scaffold != kNoScaffold) atomicAdd(intra + scaffold, (unsigned long long)s_cnt[s]);
    }
    if (t == 0) block_kept[blockIdx.x] = (long long)s_kept;
}

// one workgroup: block_first[b] = *length + the kept pairs of the workgroups before b, in place; *length += all of them
__global__ __launch_bounds__(256) void k_pairs_scan(long long* __restrict__ block_kept, int64_t n_blocks, unsigned long long* __restrict__ length)
{
    __shared__ long long s_sum[256];
    __shared__ long long s_carry;
    const int t = threadIdx.x;
    if (t == 0) s_carry = (long long)*length;
    __syncthreads();
    for (int64_t tile = 0; tile < n_blocks; tile += 256) {
        const int64_t b = tile + t;
        const long long mine = b < n_blocks ? block_kept[b] : 0;
        s_sum[t] = mine;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const long long below = t >= d ? s_sum[t - d] : 0;
            __syncthreads();
            s_sum[t] += below;
            __syncthreads();
        }
        if (b < n_blocks) block_kept[b] = s_carry + s_sum[t] - mine;
        __syncthreads();                                          // every lane has read the carry
        if (t == 255) s_carry += s_sum[255];
        __syncthreads();
    }
    if (t == 0) *length = (unsigned long long)s_carry;
}

__device__ __forceinline__ void pairs_store(const PairStore& st, long long at, int32_t sa, int64_t pa, int32_t sb, int64_t pb)
{
    if (at < 0 || at >= st.cap) return;                           // never outside the store
    st.scaf_a[at] = sa; st.pos_a[at] = pa; st.scaf_b[at] = sb; st.pos_b[at] = pb;
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void k_pairs_keep(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                    const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                    int64_t n, int64_t n_scaf, PairStore st, unsigned long long* __restrict__ length,
                                                    unsigned long long* __restrict__ intra, const long long* __restrict__ block_first)
{
    const int t = threadIdx.x;
    if (PLAIN) {
        const int64_t p = (int64_t)blockIdx.x * 256 + t;
        if (p >= n) return;
        const int32_t sa = scaf_a[p], sb = scaf_b[p];
        if (pairs_kept(sa, sb)) pairs_store(st, (long long)atomicAdd(length, 1ull), sa, pos_a[p], sb, pos_b[p]);
        else if (sa >= 0 && sa < n_scaf) atomicAdd(intra + sa, 1ull);
        return;
    }
    __shared__ unsigned int s_part[kParts];                       // kept pairs of (round, wave), then the kept pairs before it
    const int lane = t & 63, wave = t >> 6;
    const int64_t base = (int64_t)blockIdx.x * PAIRS_SLICE;
    int32_t sa[kRounds], sb[kRounds];
    unsigned long long who[kRounds];
#pragma unroll
    for (int u = 0; u < kRounds; u++) {
        const int64_t p = base + u * 256 + t;
        sa[u] = sb[u] = 0;
        if (p < n) { sa[u] = scaf_a[p]; sb[u] = scaf_b[p]; }
        who[u] = __ballot(p < n && pairs_kept(sa[u], sb[u]));
        if (lane == 0) s_part[u * 4 + wave] = (unsigned int)__popcll(who[u]);
    }
    __syncthreads();
    if (t == 0) {
        unsigned int before = 0;
        for (int k = 0; k < kParts; k++) { const unsigned int here = s_part[k]; s_part[k] = before; before += here; }
    }
    __syncthreads();
    const long long first = block_first[blockIdx.x];
#pragma unroll
    for (int u = 0; u < kRounds; u++) {
        if (!((who[u] >> lane) & 1ull)) continue;
        const int64_t p = base + u * 256 + t;
        const long long at = first + s_part[u * 4 + wave] + __popcll(who[u] & ((1ull << lane) - 1ull));
        pairs_store(st, at, sa[u], pos_a[p], sb[u], pos_b[p]);
    }
}

int64_t pairs_keep_blocks(int64_t n) { return n <= 0 ? 0 : (n + PAIRS_SLICE - 1) / PAIRS_SLICE; }

void launch_pairs_keep(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       int64_t n_scaf, const PairStore& store, void* length, void* intra, void* work, bool plain, hipStream_t s)
{
    if (n <= 0) return;
    unsigned long long* len = reinterpret_cast<unsigned long long*>(length);
    unsigned long long* in = reinterpret_cast<unsigned long long*>(intra);
    long long* blocks = reinterpret_cast<long long*>(work);
    if (plain) {
        hipLaunchKernelGGL(k_pairs_keep<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n, n_scaf,
                           store, len, in, blocks);
        return;
    }
    const int64_t n_blocks = pairs_keep_blocks(n);
    hipLaunchKernelGGL(k_pairs_count, dim3((unsigned)n_blocks), dim3(256), 0, s, scaf_a, scaf_b, n, n_scaf, in, blocks);
    hipLaunchKernelGGL(k_pairs_scan, dim3(1), dim3(256), 0, s, blocks, n_blocks, len);
    hipLaunchKernelGGL(k_pairs_keep<false>, dim3((unsigned)n_blocks), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n, n_scaf, store,
                       len, in, blocks);
}

}  // namespace hicmi
