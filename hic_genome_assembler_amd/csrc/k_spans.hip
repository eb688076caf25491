// k_spans.hip - spanning depth of an assembly from read pairs (hicmi_span_*).
//
// A placed scaffold is cut into cells of `step` bp from its left end as it lies in its sequence; the cells of all
// scaffolds are numbered in one order (span.h).  A cis pair with the cells ca < cb adds +1 at slot ca and -1 at slot cb of
// an array of unsigned 64-bit marks (the -1 in two's complement), so the inclusive prefix sum D[c] of the marks is the
// number of pairs with cell(a) <= c < cell(b): the pairs that span the boundary after cell c.  Integer adds commute:
// every kernel form, chunking and arrival order gives the same bits.
//   k_span_mark<true>   HICMI_SPANS_PLAIN=1: one thread per pair, two global 64-bit atomic adds per marking pair.
//   k_span_mark<false>  the combining form, after k_pair_stats: a 256-lane workgroup takes a slice of SPAN_SLICE pairs
//                       and sums the marks of equal slots as signed counts in an open-addressing table in LDS
//                       (SPAN_SLOTS slots of a 4-byte key and a 4-byte count).  A slice can mark 2 x SPAN_SLICE distinct
//                       slots, more than the table holds: a mark that finds neither its slot nor a free one within
//                       SPAN_PROBES probes goes to global memory directly.  Then every used slot whose count is not 0
//                       issues one global atomic add.  A sorted pair file sends a slice to very few slots.
//                       Both forms count the five kinds of pairs per wave (a ballot per kind), per workgroup in LDS, and
//                       add five numbers per workgroup to the global counters.
//   k_span_tile_sums, k_span_scan_tiles, k_span_scan_add
//                       the inclusive prefix sum of 64-bit integers in three launches: the sum of every tile of
//                       SPAN_SCAN_TILE elements; one workgroup turns the tile sums into exclusive offsets, SPAN_SCAN_WIDTH
//                       at a time with a carry; every tile is scanned again and its offset added.  No workgroup waits for
//                       another one.  Run twice: marks -> D and D -> S.
//   k_span_pick         one wave per record (lo, hi, q0, q1): lanes stride over the slots lo .. hi, keep the competing
//                       slot of lowest ratio D F / min(Lsum, Rsum) (span.h), and a wave argmin takes the lowest ratio and
//                       among equal ratios the lowest slot.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((SPAN_SLOTS & (SPAN_SLOTS - 1)) == 0 && SPAN_SLOTS == 1 << SPAN_SLOT_BITS, "the table is a power of two");
static_assert(SPAN_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");
static_assert(SPAN_SCAN_TILE == 256 * SPAN_SCAN_ITEMS && SPAN_SCAN_WIDTH % 256 == 0, "a thread scans SPAN_SCAN_ITEMS elements in a row");
static_assert(SPAN_MAX_CELLS <= (int64_t)1 << 31, "a slot is a 32-bit key of the table");

constexpr unsigned int kNoSlot = ~0u;

// one mark of `sign` at `slot`: into the table, or directly when the table has no room within SPAN_PROBES probes
__device__ __forceinline__ void span_mark_lds(unsigned int* s_key, int* s_cnt, unsigned long long* __restrict__ marks, unsigned int slot,
                                              int sign)
{
    unsigned int h = (slot * 0x9E3779B9u) >> (32 - SPAN_SLOT_BITS);
    for (int probe = 0; probe < SPAN_PROBES; probe++) {
        const unsigned int seen = atomicCAS(&s_key[h], kNoSlot, slot);
        if (seen == kNoSlot || seen == slot) { atomicAdd(&s_cnt[h], sign); return; }
        h = (h + 1) & (SPAN_SLOTS - 1);
    }
    atomicAdd(marks + slot, (unsigned long long)(long long)sign);
}

template <bool PLAIN>
__global__ __launch_bounds__(256) void k_span_mark(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                   const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                   int64_t n, LiftTables L, SpanGrid G, unsigned long long* __restrict__ marks,
                                                   unsigned long long* __restrict__ counters)
{
    __shared__ unsigned int s_key[PLAIN ? 1 : SPAN_SLOTS];
    __shared__ int s_cnt[PLAIN ? 1 : SPAN_SLOTS];
    __shared__ unsigned int s_kind[SPAN_COUNTERS];
    const int t = threadIdx.x;
    if (!PLAIN)
        for (int s = t; s < SPAN_SLOTS; s += 256) { s_key[s] = kNoSlot; s_cnt[s] = 0; }
    if (t < SPAN_COUNTERS) s_kind[t] = 0u;
    __syncthreads();
    constexpr int kPerLane = PLAIN ? 1 : SPAN_SLICE / 256;
    const int64_t base = (int64_t)blockIdx.x * (256 * kPerLane);
    for (int u = 0; u < kPerLane; u++) {
        const int64_t p = base + u * 256 + t;
        int kind = SPAN_NOWHERE;
        int64_t lo = 0, hi = 0;
        if (p < n) kind = span_classify(L, G, scaf_a[p], pos_a[p], scaf_b[p], pos_b[p], &lo, &hi);
        if (kind == SPAN_MARKED) {
            if (PLAIN) {
                atomicAdd(marks + lo, 1ull);
                atomicAdd(marks + hi, ~0ull);
            } else {
                span_mark_lds(s_key, s_cnt, marks, (unsigned int)lo, 1);
                span_mark_lds(s_key, s_cnt, marks, (unsigned int)hi, -1);
            }
        }
        // the five counters: one ballot per kind and wave (every lane of the wave is here: no lane left the loop)
#pragma unroll
        for (int k = 0; k < SPAN_COUNTERS; k++) {
            const unsigned long long who = __ballot(kind == k);
            if ((t & 63) == 0 && who) atomicAdd(&s_kind[k], (unsigned int)__popcll(who));
        }
    }
    __syncthreads();
    if (!PLAIN)
        for (int s = t; s < SPAN_SLOTS; s += 256) {
            const unsigned int slot = s_key[s];
            const int cnt = s_cnt[s];
            if (slot != kNoSlot && cnt != 0) atomicAdd(marks + slot, (unsigned long long)(long long)cnt);
        }
    if (t < SPAN_COUNTERS && s_kind[t]) atomicAdd(counters + t, (unsigned long long)s_kind[t]);
}

// ---- the prefix sum ------------------------------------------------------------------------------------------------------
// inclusive scan of the 256 values v (one per thread) through LDS; returns this thread's inclusive sum
__device__ __forceinline__ unsigned long long span_block_scan(unsigned long long v, unsigned long long* s_scan)
{
    const int t = threadIdx.x;
    s_scan[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned long long o = t >= d ? s_scan[t - d] : 0ull;
        __syncthreads();
        s_scan[t] += o;
        __syncthreads();
    }
    return s_scan[t];
}

__global__ __launch_bounds__(256) void k_span_tile_sums(const unsigned long long* __restrict__ in, int64_t n,
                                                        unsigned long long* __restrict__ tile_sums)
{
    __shared__ unsigned long long s_scan[256];
    const int64_t first = (int64_t)blockIdx.x * SPAN_SCAN_TILE + (int64_t)threadIdx.x * SPAN_SCAN_ITEMS;
    unsigned long long sum = 0ull;
#pragma unroll
    for (int k = 0; k < SPAN_SCAN_ITEMS; k++)
        if (first + k < n) sum += in[first + k];
    const unsigned long long incl = span_block_scan(sum, s_scan);
    if (threadIdx.x == 255) tile_sums[blockIdx.x] = incl;
}

// one workgroup: tile_sums[k] becomes the sum of the tiles before k
__global__ __launch_bounds__(256) void k_span_scan_tiles(unsigned long long* __restrict__ tile_sums, int64_t n_tiles)
{
    __shared__ unsigned long long s_scan[256];
    __shared__ unsigned long long s_carry;
    constexpr int kItems = SPAN_SCAN_WIDTH / 256;
    if (threadIdx.x == 0) s_carry = 0ull;
    __syncthreads();
    for (int64_t base = 0; base < n_tiles; base += SPAN_SCAN_WIDTH) {
        const int64_t first = base + (int64_t)threadIdx.x * kItems;
        unsigned long long v[kItems], sum = 0ull;
#pragma unroll
        for (int k = 0; k < kItems; k++) { v[k] = first + k < n_tiles ? tile_sums[first + k] : 0ull; sum += v[k]; }
        const unsigned long long incl = span_block_scan(sum, s_scan);
        unsigned long long run = s_carry + incl - sum;
#pragma unroll
        for (int k = 0; k < kItems; k++) {
            if (first + k < n_tiles) tile_sums[first + k] = run;
            run += v[k];
        }
        __syncthreads();                                         // every thread has read the carry
        if (threadIdx.x == 255) s_carry += incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_span_scan_add(const unsigned long long* __restrict__ in, unsigned long long* __restrict__ out,
                                                       int64_t n, const unsigned long long* __restrict__ tile_offset)
{
    __shared__ unsigned long long s_scan[256];
    const int64_t first = (int64_t)blockIdx.x * SPAN_SCAN_TILE + (int64_t)threadIdx.x * SPAN_SCAN_ITEMS;
    unsigned long long v[SPAN_SCAN_ITEMS], sum = 0ull;
#pragma unroll
    for (int k = 0; k < SPAN_SCAN_ITEMS; k++) { v[k] = first + k < n ? in[first + k] : 0ull; sum += v[k]; }
    const unsigned long long incl = span_block_scan(sum, s_scan);
    unsigned long long run = tile_offset[blockIdx.x] + incl - sum;
#pragma unroll
    for (int k = 0; k < SPAN_SCAN_ITEMS; k++) {
        run += v[k];
        if (first + k < n) out[first + k] = run;
    }
}

// ---- the picks -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_span_pick(const unsigned long long* __restrict__ D, const unsigned long long* __restrict__ S,
                                                   int64_t n_cells, int64_t F, const int64_t* __restrict__ recs, int64_t n_rec,
                                                   int64_t* __restrict__ picks)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n_rec) return;                                      // the whole wave
    const int64_t lo = recs[4 * r], hi = recs[4 * r + 1], q0 = recs[4 * r + 2], q1 = recs[4 * r + 3];
    double best = 0.0;
    long long slot = -1;
    unsigned long long depth = 0ull, lsum = 0ull, rsum = 0ull;
    // the host checked 0 <= q0 <= lo <= hi < q1 <= n_cells; a record that is not so picks nothing
    if (q0 >= 0 && q0 <= lo && hi < q1 && q1 <= n_cells)
        for (int64_t c = lo + lane; c <= hi; c += 64) {
            unsigned long long ls, rs;
            if (!span_competes(S, c, F, q0, q1, &ls, &rs)) continue;
            const double ratio = span_ratio(D[c], F, ls, rs);
            if (slot < 0 || ratio < best) { best = ratio; slot = c; depth = D[c]; lsum = ls; rsum = rs; }
        }
    for (int off = 32; off >= 1; off >>= 1) {
        const double o_best = __shfl_xor(best, off, 64);
        const long long o_slot = __shfl_xor(slot, off, 64);
        const unsigned long long o_depth = __shfl_xor(depth, off, 64), o_lsum = __shfl_xor(lsum, off, 64), o_rsum = __shfl_xor(rsum, off, 64);
        const bool take = o_slot >= 0 && (slot < 0 || o_best < best || (o_best == best && o_slot < slot));
        if (take) { best = o_best; slot = o_slot; depth = o_depth; lsum = o_lsum; rsum = o_rsum; }
    }
    if (lane == 0) {
        picks[4 * r] = slot; picks[4 * r + 1] = (int64_t)depth; picks[4 * r + 2] = (int64_t)lsum; picks[4 * r + 3] = (int64_t)rsum;
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------
void launch_span_mark(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                      const LiftTables& lift, const SpanGrid& grid, void* marks, void* counters, bool plain, hipStream_t s)
{
    if (n <= 0) return;
    unsigned long long* m = reinterpret_cast<unsigned long long*>(marks);
    unsigned long long* k = reinterpret_cast<unsigned long long*>(counters);
    if (plain)
        hipLaunchKernelGGL(k_span_mark<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n, lift,
                           grid, m, k);
    else
        hipLaunchKernelGGL(k_span_mark<false>, dim3((unsigned)((n + SPAN_SLICE - 1) / SPAN_SLICE)), dim3(256), 0, s, scaf_a, pos_a,
                           scaf_b, pos_b, n, lift, grid, m, k);
}

int64_t span_scan_tiles(int64_t n) { return (n + SPAN_SCAN_TILE - 1) / SPAN_SCAN_TILE; }

void launch_span_scan(const void* in, void* out, int64_t n, void* tile_sums, hipStream_t s)
{
    if (n <= 0) return;
    const int64_t tiles = span_scan_tiles(n);
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(in);
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(tile_sums);
    hipLaunchKernelGGL(k_span_tile_sums, dim3((unsigned)tiles), dim3(256), 0, s, src, n, sums);
    hipLaunchKernelGGL(k_span_scan_tiles, dim3(1), dim3(256), 0, s, sums, tiles);
    hipLaunchKernelGGL(k_span_scan_add, dim3((unsigned)tiles), dim3(256), 0, s, src, reinterpret_cast<unsigned long long*>(out), n, sums);
}

void launch_span_pick(const void* depth, const void* depth_sums, int64_t n_cells, int64_t flank, const int64_t* recs, int64_t n_rec,
                      int64_t* picks, hipStream_t s)
{
    if (n_rec <= 0) return;
    hipLaunchKernelGGL(k_span_pick, dim3((unsigned)((n_rec + 3) / 4)), dim3(256), 0, s, reinterpret_cast<const unsigned long long*>(depth),
                       reinterpret_cast<const unsigned long long*>(depth_sums), n_cells, flank, recs, n_rec, picks);
}

}  // namespace hicmi
