// k_split.hip - read pairs moved from scaffolds to the pieces the scaffolds are cut into (hicmi_split_*).
//
// A chunk of pairs (scaffold, position) x 2 is rewritten in place to (piece, position in the piece) by split.h's rule, and
// every pair adds to the counters of its pieces, [within][sibling][other][mark] x n_piece unsigned 64-bit integers (a mark
// of -1 in two's complement).  Integer adds commute: both forms, every chunking and every arrival order give the same bits.
//   k_split_pairs<true>   HICMI_SPLIT_PLAIN=1, the definition taken literally: a scan over the pieces of the scaffold, one
//                         global 64-bit atomic add per counter and pair.
//   k_split_pairs<false>  the default: an uncut scaffold is its one piece, a cut one is searched by bisection; the
//                         workgroup sums the contributions of equal counters as signed counts in an open-addressing table
//                         in LDS (SPLIT_SLOTS slots of a 4-byte key and a 4-byte count) over all the slices of SPLIT_SLICE
//                         pairs it takes, and issues one global atomic add per used counter at its end.  A contribution
//                         that finds neither its counter nor a free slot within SPLIT_PROBES probes goes to global memory
//                         directly.  A sorted pair file sends a workgroup to very few counters.
// Both are 256-thread workgroups in a grid-stride loop over at most SPLIT_MAX_BLOCKS workgroups.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((SPLIT_SLOTS & (SPLIT_SLOTS - 1)) == 0 && SPLIT_SLOTS == 1 << SPLIT_SLOT_BITS, "the table is a power of two");
static_assert(SPLIT_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");

constexpr unsigned int kNoCounter = ~0u;

// `add` at counter `idx`: into the table, or directly when the table has no room within SPLIT_PROBES probes
__device__ __forceinline__ void split_add_lds(unsigned int* s_key, int* s_cnt, unsigned long long* counters, unsigned int idx, int add)
{
    unsigned int h = (idx * 0x9E3779B9u) >> (32 - SPLIT_SLOT_BITS);
    for (int probe = 0; probe < SPLIT_PROBES; probe++) {
        const unsigned int seen = atomicCAS(&s_key[h], kNoCounter, idx);
        if (seen == kNoCounter || seen == idx) { atomicAdd(&s_cnt[h], add); return; }
        h = (h + 1) & (SPLIT_SLOTS - 1);
    }
    atomicAdd(counters + idx, (unsigned long long)(long long)add);
}

// scaf_* and pos_* are read and written at the same index by the same thread: in place
template <bool PLAIN>
__global__ __launch_bounds__(256) void k_split_pairs(int32_t* scaf_a, int64_t* pos_a, int32_t* scaf_b, int64_t* pos_b, int64_t n,
                                                     SplitTables T, unsigned long long* counters)
{
    __shared__ unsigned int s_key[PLAIN ? 1 : SPLIT_SLOTS];
    __shared__ int s_cnt[PLAIN ? 1 : SPLIT_SLOTS];
    const int t = threadIdx.x;
    if (!PLAIN) {
        for (int s = t; s < SPLIT_SLOTS; s += 256) { s_key[s] = kNoCounter; s_cnt[s] = 0; }
        __syncthreads();
    }
    constexpr int64_t kSlice = PLAIN ? 256 : SPLIT_SLICE;
    for (int64_t base = (int64_t)blockIdx.x * kSlice; base < n; base += (int64_t)gridDim.x * kSlice) {
#pragma unroll 1
        for (int u = 0; u < kSlice / 256; u++) {
            const int64_t p = base + u * 256 + t;
            if (p >= n) break;
            const int32_t sa = scaf_a[p], sb = scaf_b[p];
            // the host checked every index and position before the chunk was uploaded; a pair that is not so is left alone
            if (sa < 0 || sa >= T.n_scaf || sb < 0 || sb >= T.n_scaf) continue;
            int64_t xa, xb;
            const int32_t ka = PLAIN ? split_end_scan(T, sa, pos_a[p], &xa) : split_end(T, sa, pos_a[p], &xa);
            const int32_t kb = PLAIN ? split_end_scan(T, sb, pos_b[p], &xb) : split_end(T, sb, pos_b[p], &xb);
            scaf_a[p] = ka; pos_a[p] = xa; scaf_b[p] = kb; pos_b[p] = xb;
            int64_t idx[4];
            int add[4];
            const int m = split_contributions(T.n_piece, sa, ka, sb, kb, idx, add);
            for (int q = 0; q < m; q++) {
                if (PLAIN) atomicAdd(counters + idx[q], (unsigned long long)(long long)add[q]);
                else split_add_lds(s_key, s_cnt, counters, (unsigned int)idx[q], add[q]);
            }
        }
    }
    if (!PLAIN) {
        __syncthreads();
        for (int s = t; s < SPLIT_SLOTS; s += 256) {
            const unsigned int idx = s_key[s];
            const int cnt = s_cnt[s];
            if (idx != kNoCounter && cnt != 0) atomicAdd(counters + idx, (unsigned long long)(long long)cnt);
        }
    }
}

// The chunk is rewritten in place; counters: 4 n_piece cells the contributions are added to.  4 n_piece < 2^32 (the host
// checks it): a counter is a 32-bit key of the table.
void launch_split_pairs(int32_t* scaf_a, int64_t* pos_a, int32_t* scaf_b, int64_t* pos_b, int64_t n, const SplitTables& tables,
                        void* counters, bool plain, hipStream_t s)
{
    if (n <= 0) return;
    unsigned long long* k = reinterpret_cast<unsigned long long*>(counters);
    if (plain) {
        const int64_t blocks = std::min<int64_t>((n + 255) / 256, SPLIT_MAX_BLOCKS);
        hipLaunchKernelGGL(k_split_pairs<true>, dim3((unsigned)blocks), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n, tables, k);
    } else {
        const int64_t blocks = std::min<int64_t>((n + SPLIT_SLICE - 1) / SPLIT_SLICE, SPLIT_MAX_BLOCKS);
        hipLaunchKernelGGL(k_split_pairs<false>, dim3((unsigned)blocks), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n, tables, k);
    }
}

}  // namespace hicmi
