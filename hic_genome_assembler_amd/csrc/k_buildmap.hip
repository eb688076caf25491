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
// A lifted build (hicmi_map_begin_lifted, hicmi_lift_maps) counts the map of the assembled genome: both
// counting kernels are templates on LIFTED, and the lifted form sends each end through the per-scaffold lift tables
// (sequence, offset, reversed; liftmap.h) before the same key arithmetic, with first_bin describing the sequences.
//   k_pair_stats        the cis / trans split per sequence and the contact-decay histogram of a chunk of pairs under a
//                       lift, combined in LDS like k_buildmap_combine (up to two 32-bit keys per pair).
// The host checks every scaffold index and position before a chunk is uploaded; the kernels still drop a pair whose
// bin would fall outside the map, so a wrong input cannot write out of bounds.
#include "hicmi_internal.h"

namespace hicmi {

static_assert((BUILDMAP_SLOTS & (BUILDMAP_SLOTS - 1)) == 0 && BUILDMAP_SLOTS >= 2 * BUILDMAP_SLICE,
              "the table is a power of two and at most half full");
static_assert(BUILDMAP_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");

static_assert((PAIRSTATS_SLOTS & (PAIRSTATS_SLOTS - 1)) == 0 && PAIRSTATS_SLOTS >= 4 * PAIRSTATS_SLICE,
              "two keys per pair, and the table is a power of two and at most half full");
static_assert(PAIRSTATS_SLICE % 256 == 0, "lane t takes the pairs t, t + 256, ... of a slice");

// the key of pair p, or kNoKey for a pair outside the map.  LIFTED: both ends go through the lift tables first, and
// first_bin / n_grid describe the assembled sequences; that is the only difference (map_cell_key, liftmap.h)
template <bool LIFTED>
__device__ __forceinline__ unsigned long long buildmap_key(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                           const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                           int64_t p, const int32_t* __restrict__ first_bin, int n_grid,
                                                           int64_t r, int m, const LiftTables& L)
{
    int32_t ga = scaf_a[p], gb = scaf_b[p];
    int64_t xa = pos_a[p], xb = pos_b[p];
    if (LIFTED) {
        int32_t qa, qb;
        int64_t ya, yb;
        if (!lift_end(L, ga, xa, &qa, &ya) || !lift_end(L, gb, xb, &qb, &yb)) return kNoKey;
        ga = qa; gb = qb; xa = ya; xb = yb;
    }
    return map_cell_key(ga, xa, gb, xb, first_bin, n_grid, r, m);
}

template <bool LIFTED>
__global__ __launch_bounds__(256) void k_buildmap_plain(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                        const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                        int64_t n, const int32_t* __restrict__ first_bin, int n_grid,
                                                        int64_t r, int m, unsigned long long* __restrict__ counts, LiftTables L)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const unsigned long long key = buildmap_key<LIFTED>(scaf_a, pos_a, scaf_b, pos_b, p, first_bin, n_grid, r, m, L);
    if (key != kNoKey) atomicAdd(counts + key, 1ull);
}

template <bool LIFTED>
__global__ __launch_bounds__(256) void k_buildmap_combine(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                          const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                          int64_t n, const int32_t* __restrict__ first_bin, int n_grid,
                                                          int64_t r, int m, unsigned long long* __restrict__ counts, LiftTables L)
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
        const unsigned long long key = buildmap_key<LIFTED>(scaf_a, pos_a, scaf_b, pos_b, p, first_bin, n_grid, r, m, L);
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

// The statistics of a chunk of pairs under a lift, added to out[256 + 2 n_seq + 1]: the decay histogram,
// cis per sequence, trans per sequence, the unlifted pairs.  The combining scheme of k_buildmap_combine with up to two
// keys per pair in one key space - a cis pair its decay slot and 256 + seq, a trans pair 256 + n_seq + seq of either end,
// an unlifted pair the last counter - and 32-bit keys: a slice of PAIRSTATS_SLICE pairs has at most 2 x PAIRSTATS_SLICE
// distinct keys in PAIRSTATS_SLOTS >= twice as many slots.  A single chromosome sends most pairs of a slice to one
// counter: they meet in LDS, and every used slot issues one 64-bit global atomic add.
constexpr unsigned int kNoStat = ~0u;

__device__ __forceinline__ void pair_stats_count(unsigned int* s_key, unsigned int* s_cnt, unsigned int key)
{
    unsigned int h = (key * 0x9E3779B9u) >> (32 - PAIRSTATS_SLOT_BITS);
    for (;;) {
        const unsigned int seen = atomicCAS(&s_key[h], kNoStat, key);
        if (seen == kNoStat || seen == key) { atomicAdd(&s_cnt[h], 1u); return; }
        h = (h + 1) & (PAIRSTATS_SLOTS - 1);
    }
}

__global__ __launch_bounds__(256) void k_pair_stats(const int32_t* __restrict__ scaf_a, const int64_t* __restrict__ pos_a,
                                                    const int32_t* __restrict__ scaf_b, const int64_t* __restrict__ pos_b,
                                                    int64_t n, LiftTables L, unsigned long long* __restrict__ out)
{
    __shared__ unsigned int s_key[PAIRSTATS_SLOTS];
    __shared__ unsigned int s_cnt[PAIRSTATS_SLOTS];
    const int t = threadIdx.x;
    for (int s = t; s < PAIRSTATS_SLOTS; s += 256) { s_key[s] = kNoStat; s_cnt[s] = 0u; }
    __syncthreads();
    const unsigned int k_cis = LIFT_DECAY_SLOTS, k_trans = k_cis + (unsigned int)L.n_seq, k_unlifted = k_trans + (unsigned int)L.n_seq;
    const int64_t base = (int64_t)blockIdx.x * PAIRSTATS_SLICE;
    for (int u = 0; u < PAIRSTATS_SLICE / 256; u++) {
        const int64_t p = base + u * 256 + t;
        if (p >= n) break;
        int32_t qa, qb;
        int64_t ya = 0, yb = 0;
        const bool ok_a = lift_end(L, scaf_a[p], pos_a[p], &qa, &ya), ok_b = lift_end(L, scaf_b[p], pos_b[p], &qb, &yb);
        if (!ok_a || !ok_b) {
            // an end on a dropped scaffold; an end outside the tables (the host refuses those) counts nowhere
            if (qa >= -1 && qb >= -1) pair_stats_count(s_key, s_cnt, k_unlifted);
            continue;
        }
        if (qa == qb) {
            const uint64_t d = ya < yb ? (uint64_t)(yb - ya) : (uint64_t)(ya - yb);
            pair_stats_count(s_key, s_cnt, (unsigned int)lift_decay_slot(d));
            pair_stats_count(s_key, s_cnt, k_cis + (unsigned int)qa);
        } else {
            pair_stats_count(s_key, s_cnt, k_trans + (unsigned int)qa);
            pair_stats_count(s_key, s_cnt, k_trans + (unsigned int)qb);
        }
    }
    __syncthreads();
    for (int s = t; s < PAIRSTATS_SLOTS; s += 256) {
        const unsigned int key = s_key[s];
        if (key != kNoStat) atomicAdd(out + key, (unsigned long long)s_cnt[s]);
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

template <bool LIFTED>
static void launch_add(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       const int32_t* first_bin, int n_grid, int64_t r, int m, unsigned long long* cnt, bool plain,
                       const LiftTables& L, hipStream_t s)
{
    if (plain)
        hipLaunchKernelGGL(k_buildmap_plain<LIFTED>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, scaf_a, pos_a, scaf_b, pos_b,
                           n, first_bin, n_grid, r, m, cnt, L);
    else
        hipLaunchKernelGGL(k_buildmap_combine<LIFTED>, dim3((unsigned)((n + BUILDMAP_SLICE - 1) / BUILDMAP_SLICE)), dim3(256), 0, s,
                           scaf_a, pos_a, scaf_b, pos_b, n, first_bin, n_grid, r, m, cnt, L);
}

void launch_buildmap_add(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                         const int32_t* first_bin, int n_grid, int64_t r, int m, void* counts, bool plain, const LiftTables& lift,
                         hipStream_t s)
{
    if (n <= 0) return;
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
    if (lift.seq) launch_add<true>(scaf_a, pos_a, scaf_b, pos_b, n, first_bin, n_grid, r, m, cnt, plain, lift, s);
    else launch_add<false>(scaf_a, pos_a, scaf_b, pos_b, n, first_bin, n_grid, r, m, cnt, plain, lift, s);
}

void launch_pair_stats(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       const LiftTables& lift, void* out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pair_stats, dim3((unsigned)((n + PAIRSTATS_SLICE - 1) / PAIRSTATS_SLICE)), dim3(256), 0, s, scaf_a, pos_a,
                       scaf_b, pos_b, n, lift, reinterpret_cast<unsigned long long*>(out));
}

void launch_buildmap_finish(void* cells, int m, hipStream_t s)
{
    const unsigned tiles = (unsigned)((m + 63) / 64);
    hipLaunchKernelGGL(k_buildmap_finish, dim3(tiles, tiles), dim3(256), 0, s, cells, m);
}

}  // namespace hicmi
