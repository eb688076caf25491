// k_part2_invert.hip - segment-inversion support of a finished Part 2 ordering (hicmi_p2_inversions_multi).
//
// Candidate (i, j), 0 <= i <= j < S, of a chromosome's final arrangement A is A with its positions [a, b) =
// [arr_pos[i], arr_pos[j + 1]) read backwards: scaffolds i ... j in reverse order, each flipped.  Pairs inside the
// segment and pairs outside it keep their distance, so with c = a + b - 1 (position t of the segment moves to c - t)
//     total * (score(i, j) - score0) = sum_{t in [a, b)} [ sum_{o < a}  M[t][o] * (h(c - t - o) - h(t - o))
//                                                         + sum_{o >= b} M[t][o] * (h(o + t - c) - h(o - t)) ],
//     h(d) = H[n - 1] - H[d - 1],   so   h(new) - h(old) = H[old - 1] - H[new - 1].
// One InvRec per (chromosome, left end i), built by the host for the whole genome.  Two launches:
//   k_inv_tables  a flat grid; every record owns the workgroups [wg0, next record's wg0) and a workgroup finds its
//                 record by bisection.  The first record of a chromosome owns INV_BASE_SLABS workgroups for the BASE
//                 slabs of A (base_partial_body); then ONE workgroup per right end j = i ... i + n_j - 1: its four waves
//                 take the rows t of the segment in turn, the lanes the positions o outside it, and block_sum_256 adds
//                 the 256 partial sums in its fixed order: the same bits from run to run, no atomics, no scratch.
//   k_inv_scores  one workgroup per record: BASE = the slabs left to right, row i of the table (BASE + sum) / total
//                 (0.0 left of the diagonal and beyond max_span), and the record's pick (pick_first_max_256,
//                 hicmi_internal.h) over the candidates of inv_counts.
// No candidate bin order is built.  Matrix reads per chromosome: the sum over the computed candidates of
// len * (n - len), len = b - a; the host adds that up before the launch and refuses a call above INV_MAX_WORK.
//
// LDS: neither kernel has dynamic LDS or stages anything whose size depends on a record - the arrangement, the rows and
// H are read from global memory (L1 / L2) - so every workgroup takes the same path and a launch that mixes a chromosome
// of a few bins with one of thousands has no threshold to fall on either side of.
#include "hicmi_internal.h"

namespace hicmi {

// a candidate that competes: a segment of at least two scaffolds that is not the whole chromosome (read backwards it
// has the same objective) and is not wider than max_span (0: no limit).  j = i is placement support's in-place flip.
__device__ __forceinline__ bool inv_counts(int i, int j, int S, int max_span)
{
    if (j <= i) return false;
    if (i == 0 && j == S - 1) return false;
    return max_span <= 0 || j - i + 1 <= max_span;
}

__global__ __launch_bounds__(256) void k_inv_tables(const InvRec* __restrict__ recs, int n_rec)
{
    __shared__ double s_w[4];
    const int64_t bx0 = blockIdx.x;
    int lo = 0, hi = n_rec - 1;                          // the last record whose first workgroup is at or before this one
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].wg0 <= bx0) lo = mid; else hi = mid - 1;
    }
    const InvRec& d = recs[lo];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = d.n;
    const int32_t* __restrict__ pos = d.pos;
    const double* __restrict__ H = d.H;
    int64_t bx = bx0 - d.wg0;
    if (bx < d.n_base) {
        base_partial_body(d.M2, d.ld2, pos, n, H, n, (int)bx, d.n_base, d.base + bx);
        return;
    }
    bx -= d.n_base;
    if (bx >= d.n_j) return;
    const int j = d.i + (int)bx;
    const int a = d.arr_pos[d.i], b = d.arr_pos[j + 1], c = a + b - 1;
    double acc = 0.0;
    for (int t = a + wave; t < b; t += 4) {
        const double* __restrict__ row = d.M2 + (int64_t)pos[t] * d.ld2;
        const int q = c - t;                             // where position t lies after the reversal
#pragma unroll 4
        for (int o = lane; o < a; o += 64) acc += row[pos[o]] * (H[t - o - 1] - H[q - o - 1]);
#pragma unroll 4
        for (int o = b + lane; o < n; o += 64) acc += row[pos[o]] * (H[o - t - 1] - H[o - q - 1]);
    }
    const double sum = block_sum_256(acc, s_w);
    if (threadIdx.x == 0) d.scores[j] = sum;
}

__global__ __launch_bounds__(256) void k_inv_scores(const InvRec* __restrict__ recs, double near_top)
{
    __shared__ double s_part[INV_BASE_SLABS], s_base;
    const InvRec& d = recs[blockIdx.x];
    const int tid = threadIdx.x, S = d.S, i = d.i, n_j = d.n_j, max_span = d.max_span;
    for (int k = tid; k < INV_BASE_SLABS; k += 256) s_part[k] = d.base[k];
    __syncthreads();
    if (tid == 0) s_base = serial_sum_lds(s_part, 0, INV_BASE_SLABS, 0.0);
    __syncthreads();
    const double base = s_base, total = d.total;
    double* __restrict__ row = d.scores;
    for (int j = tid; j < S; j += 256) row[j] = (j >= i && j - i < n_j) ? (base + row[j]) / total : 0.0;
    pick_first_max_256(tid, S, row, d.best, near_top, [=](int j) { return inv_counts(i, j, S, max_span); });
}

void launch_inv(const InvRec* recs, int n_rec, int64_t n_wg, double near_top, hipStream_t s)
{
    hipLaunchKernelGGL(k_inv_tables, dim3((unsigned)n_wg), dim3(256), 0, s, recs, n_rec);
    hipLaunchKernelGGL(k_inv_scores, dim3(n_rec), dim3(256), 0, s, recs, near_top);
}

}  // namespace hicmi
