// k_junctions.hip - junction support of a finished ordering (hicmi_junction_sums).
//
// A record r is a pair of sides (A, B) of one junction: side entry k is the matrix index bins[start + k * step],
// step = +1 or -1, entry 0 touching the junction.  Wanted per record:
//     sum(A, B) = sum over a < lenA, b < lenB of M[A_a][B_b] * w[a + b + 1],   w[d] = 1.0 / d from the host's table
// (the kernels never divide).  The product is rounded before it is added (-ffp-contract=off).  Every chromosome's bin
// order is uploaded once per call as `bins`; the sides are views of it and nothing is copied per record.
//   k_junctions_partial  a flat grid; record r owns the workgroups [wg0, wg0 + n_slabs), one per slab of JN_SLAB_ROWS rows
//                        of A (the last slab is shorter), and a workgroup finds its record by bisection.  The slab's
//                        rows x lenB elements are numbered row-major; lane t takes the elements t, t + 256, ... in
//                        ascending order - (a, b) advance by (256 / lenB, 256 % lenB) with one carry, so the loop has
//                        no division - and block_sum_256 adds the 256 lane sums in its fixed order.
//   k_junctions_reduce   one lane per record: its slab partials left to right from 0.0.
//   k_junctions_plain    HICMI_JUNCTIONS_PLAIN=1, the A/B and the definition taken literally: one lane per record, a
//                        outer and b inner, one running sum.
// The order of every sum is fixed by (lenA, lenB) alone: two calls give the same bits, whatever else is in the call.
//
// LDS: the four doubles of block_sum_256.  No dynamic LDS and no staging whose size depends on a record - sides, rows
// and weights are read from global memory (L1 / L2) - so a 1 x 1 record and a 1,900 x 1,900 one take the same path and a
// call that mixes them has no threshold to straddle (the discipline of DESIGN.md 9j).  No atomics.
#include "hicmi_internal.h"

namespace hicmi {

__global__ __launch_bounds__(256) void k_junctions_partial(const double* __restrict__ C, int64_t ld,
                                                           const int32_t* __restrict__ bins, const JnRec* __restrict__ recs,
                                                           int n_rec, const double* __restrict__ w,
                                                           double* __restrict__ partial)
{
    __shared__ double s_w[4];
    const int64_t bx0 = blockIdx.x;
    int lo = 0, hi = n_rec - 1;                          // the last record whose first workgroup is at or before this one
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].wg0 <= bx0) lo = mid; else hi = mid - 1;
    }
    const JnRec d = recs[lo];
    const int a0 = (int)(bx0 - d.wg0) * JN_SLAB_ROWS;
    const int rows = min(JN_SLAB_ROWS, d.lenA - a0), lenB = d.lenB;
    const int q = 256 / lenB, rm = 256 - q * lenB;
    int a = (int)threadIdx.x / lenB, b = (int)threadIdx.x - a * lenB;
    const int32_t* __restrict__ sideA = bins + d.startA + (int64_t)a0 * d.stepA;
    const int32_t* __restrict__ sideB = bins + d.startB;
    const double* __restrict__ wd = w + a0 + 1;
    double acc = 0.0;
    while (a < rows) {
        const double v = C[(int64_t)sideA[(int64_t)a * d.stepA] * ld + sideB[(int64_t)b * d.stepB]];
        acc += v * wd[a + b];
        a += q; b += rm;
        if (b >= lenB) { b -= lenB; a++; }
    }
    const double sum = block_sum_256(acc, s_w);
    if (threadIdx.x == 0) partial[bx0] = sum;
}

__global__ __launch_bounds__(256) void k_junctions_reduce(const JnRec* __restrict__ recs, int n_rec,
                                                          const double* __restrict__ partial, double* __restrict__ sums)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    const JnRec d = recs[r];
    const double* __restrict__ p = partial + d.wg0;
    double acc = 0.0;
    for (int s = 0; s < d.n_slabs; s++) acc += p[s];
    sums[r] = acc;
}

__global__ __launch_bounds__(256) void k_junctions_plain(const double* __restrict__ C, int64_t ld,
                                                         const int32_t* __restrict__ bins, const JnRec* __restrict__ recs,
                                                         int n_rec, const double* __restrict__ w, double* __restrict__ sums)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rec) return;
    const JnRec d = recs[r];
    double acc = 0.0;
    for (int a = 0; a < d.lenA; a++) {
        const double* __restrict__ row = C + (int64_t)bins[d.startA + (int64_t)a * d.stepA] * ld;
        for (int b = 0; b < d.lenB; b++) acc += row[bins[d.startB + (int64_t)b * d.stepB]] * w[a + b + 1];
    }
    sums[r] = acc;
}

void launch_junction_sums(const double* C, int64_t ld, const int32_t* bins, const JnRec* recs, int n_rec, int64_t n_wg,
                          const double* w, double* partial, double* sums, bool plain, hipStream_t s)
{
    const unsigned per_rec = (unsigned)((n_rec + 255) / 256);
    if (plain) {
        hipLaunchKernelGGL(k_junctions_plain, dim3(per_rec), dim3(256), 0, s, C, ld, bins, recs, n_rec, w, sums);
        return;
    }
    hipLaunchKernelGGL(k_junctions_partial, dim3((unsigned)n_wg), dim3(256), 0, s, C, ld, bins, recs, n_rec, w, partial);
    hipLaunchKernelGGL(k_junctions_reduce, dim3(per_rec), dim3(256), 0, s, recs, n_rec, partial, sums);
}

}  // namespace hicmi
