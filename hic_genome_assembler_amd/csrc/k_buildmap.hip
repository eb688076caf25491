// k_buildmap.hip - a raw contact map counted from read pairs (hicmi_map_*, hicmi_build_maps): the device
// side of a HiC-Pro `build_matrix` run at any bin size.
//
// A pair is (scaffold a, position a, scaffold b, position b), positions 1-based.  Its ends fall in the bins
//   i = first_bin[a] + (pos_a - 1) / r,   j = first_bin[b] + (pos_b - 1) / r
// and it adds 1 to the cell (min(i, j), max(i, j)) of an m x m array of unsigned 64-bit counts: only the upper triangle
// with the diagonal is counted.  Integer adds commute, so every kernel here and every arrival order give the same bits.
//   k_buildmap_plain    the default: one thread per pair, one global atomic add of 1 per pair - the definition taken
//                       literally.
//   k_buildmap_combine  HICMI_BUILDMAP_PLAIN=0, the A/B.  HiC-Pro's merged pair file is sorted by (scaffold1, pos1) and
//                       contacts pile up near the diagonal, so neighbouring pairs can hit the same few cells.  A 256-lane
//                       workgroup takes a contiguous slice of BUILDMAP_SLICE pairs, forms the keys lo * m + hi and counts
//                       equal keys in an open-addressing hash table in LDS (BUILDMAP_SLOTS = 2 x slice slots of an 8-byte
//                       key and a 4-byte count: never more than half full, whatever m and the chunk are); then every
//                       used slot issues one global 64-bit atomic add of its multiplicity.  On the 16,000-bin bench map
//                       8.0 M sorted pairs fall into 7.5 M distinct cells: nothing to combine, and it measured 541 us
//                       against the plain kernel's 465 us, which is why it is not the default.
//   k_buildmap_finish   afterwards, in place: the counts of the upper triangle become doubles (exact below 2^53) and the
//                       strict upper triangle is mirrored into the lower one, 64 x 64 tiles through LDS like
//                       k_rebin_mirror.  A count and its double are both 8 bytes: the cell (r, c), r <= c, is read and
//                       rewritten by one lane, and the lower triangle is never read.
// The host checks every scaffold index and position before a chunk is uploaded; the kernels still drop a pair whose
// bin would fall outside the map, so a wrong input cannot write out of bounds.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((BUILDMAP_SLOTS & (BUILDMAP_SLOTS - 1)) == 0 && BUILDMAP_SLOTS >= 2 * BUILDMAP_SLICE,
              "the table is a power of two and at most half full");
static_assert(BUILDMAP_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");

constexpr unsigned long long kNoKey = ~0ull;      // lo * m + hi <= 2^32 - 1 for m <= 65536

// the key of pair p, or kNoKey for a pair outside the map
__device__ __forceinline__ unsigned long long buildmap_key(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                           const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                           int64_t p, const int32_t* __restrict__ first_bin, int n_scaf,
                                                           int64_t r, int m)
{
    const int32_t sa = scaf_a[p], sb = scaf_b[p];
    const int64_t pa = pos_a[p] - 1, pb = pos_b[p] - 1;
    if (sa < 0 || sa >= n_scaf || sb < 0 || sb >= n_scaf || pa < 0 || pb < 0) return kNoKey;
    int64_t ka, kb;
    if (((uint64_t)pa | (uint64_t)pb | (uint64_t)r) >> 32) { ka = pa / r; kb = pb / r; }
    else { ka = (uint32_t)pa / (uint32_t)r; kb = (uint32_t)pb / (uint32_t)r; }      // the usual case: 32-bit division
    const int64_t i = first_bin[sa] + ka, j = first_bin[sb] + kb;
    if (i >= m || j >= m) return kNoKey;
    const int64_t lo = i < j ? i : j, hi = i < j ? j : i;
    return (unsigned long long)(lo * m + hi);
}

__global__ __launch_bounds__(256) void k_buildmap_plain(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                        const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                        int64_t n, const int32_t* __restrict__ first_bin, int n_scaf,
                                                        int64_t r, int m, unsigned long long* __restrict__ counts)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const unsigned long long key = buildmap_key(scaf_a, pos_a, scaf_b, pos_b, p, first_bin, n_scaf, r, m);
    if (key != kNoKey) atomicAdd(counts + key, 1ull);
}

__global__ __launch_bounds__(256) void k_buildmap_combine(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                          const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                          int64_t n, const int32_t* __restrict__ first_bin, int n_scaf,
                                                          int64_t r, int m, unsigned long long* __restrict__ counts)
{
    __shared__ unsigned long long s_key[BUILDMAP_SLOTS];
    __shared__ unsigned int s_cnt[BUILDMAP_SLOTS];
    const int t = threadIdx.x;
    for (int s = t; s < BUILDMAP_SLOTS; s += 256) { s_key[s] = kNoKey; s_cnt[s] = 0u; }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * BUILDMAP_SLICE;
#pragma unroll 2
    for (int u = 0; u < BUILDMAP_SLICE / 256; u++) {
        const int64_t p = base + u * 256 + t;
        if (p >= n) break;
        const unsigned long long key = buildmap_key(scaf_a, pos_a, scaf_b, pos_b, p, first_bin, n_scaf, r, m);
        if (key == kNoKey) continue;
        // Fibonacci hashing, then linear probing: at most BUILDMAP_SLICE distinct keys in 2 x BUILDMAP_SLICE slots, so
        // a free or matching slot always comes
        unsigned int h = (unsigned int)((key * 0x9E3779B97F4A7C15ull) >> 32) & (BUILDMAP_SLOTS - 1);
        for (;;) {
            const unsigned long long seen = atomicCAS(&s_key[h], kNoKey, key);
            if (seen == kNoKey || seen == key) { atomicAdd(&s_cnt[h], 1u); break; }
            h = (h + 1) & (BUILDMAP_SLOTS - 1);
        }
    }
    __syncthreads();
    for (int s = t; s < BUILDMAP_SLOTS; s += 256) {
        const unsigned long long key = s_key[s];
        if (key != kNoKey) atomicAdd(counts + key, (unsigned long long)s_cnt[s]);
    }
}

// in place: `cells` holds counts on entry (only r <= c is read) and the symmetric matrix of doubles on exit
__global__ __launch_bounds__(256) void k_buildmap_finish(void* __restrict__ cells, int m)
{
    __shared__ double tile[64][65];
    const unsigned long long* U = reinterpret_cast<const unsigned long long*>(cells);
    double* D = reinterpret_cast<double*>(cells);
    const int bi = blockIdx.y, bj = blockIdx.x;               // the upper tile (bi, bj) also fills the lower tile (bj, bi)
    if (bj < bi) return;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = bi * 64 + i, c = bj * 64 + tx;
        double v = 0.0;
        if (r < m && c < m && r <= c) {
            v = (double)U[(int64_t)r * m + c];
            D[(int64_t)r * m + c] = v;
        }
        tile[i][tx] = v;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int r = bj * 64 + i, c = bi * 64 + tx;
        if (r < m && c < r) D[(int64_t)r * m + c] = tile[tx][i];
    }
}

void launch_buildmap_add(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                         const int32_t* first_bin, int n_scaf, int64_t r, int m, void* counts, bool plain, hipStream_t s)
{
    if (n <= 0) return;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (plain)
        hipLaunchKernelGGL(k_buildmap_plain, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b, n,
                           first_bin, n_scaf, r, m, cnt);
    else
        hipLaunchKernelGGL(k_buildmap_combine, dim3((unsigned)((n + BUILDMAP_SLICE - 1) / BUILDMAP_SLICE)), dim3(256), 0, s,
                           scaf_a, pos_a, scaf_b, pos_b, n, first_bin, n_scaf, r, m, cnt);
}

void launch_buildmap_finish(void* cells, int m, hipStream_t s)
{
    const unsigned tiles = (unsigned)((m + 63) / 64);
    hipLaunchKernelGGL(k_buildmap_finish, dim3(tiles, tiles), dim3(256), 0, s, cells, m);
}

}  // namespace hicmi
