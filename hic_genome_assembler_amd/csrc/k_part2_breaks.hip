// k_part2_breaks.hip - break support of a finished Part 2 ordering (hicmi_p2_breaks_multi).
//
// Scaffold j of a chromosome's final arrangement A occupies L positions [B, B + L) of A, read as laid down.  Cut
// p = 1 ... L - 1 splits them into P (the first p) and Q (the rest), and candidate k = 4 w + 2 x + y swaps the pieces
// (w), reverses P (x) and reverses Q (y) in place: 8 (L - 1) candidates per scaffold, all other positions unchanged.
// Pairs inside one piece and pairs outside the block keep their distance, so with pos / newpos the positions in A and
// in the candidate
//     total * (score(p, k) - score0) = sum_{t in block} [X[t][newpos_t] - X[t][pos_t]] + PQ(p, k),
//     X[t][q]  = sum_{o outside the block} M[bin_t][bin_o] * h(|B + q - o|),         h(d) = H[n - 1] - H[d - 1],
//     PQ(p, k) = sum_{a in P, b in Q} M[a][b] * (h(d') - h(d)).
// d' is one of four functions of the pair: d (k = 0, 7), L - d (k = 3, 4), L - 1 - a - b (k = 1, 6) and a + b + 1
// (k = 2, 5), a and b counted inside their pieces, so a cut has three P x Q sums to form.
// One BrkRec per (chromosome, scaffold with L >= 2), built by the host for the whole genome.  Two launches:
//   k_brk_tables  a flat grid; every record owns the workgroups [wg0, next record's wg0) and a workgroup finds its
//                 record by bisection.  The first record of a chromosome owns BRK_BASE_SLABS workgroups for the BASE
//                 slabs of A (base_partial_body); then L * ceil(L / 4) workgroups, one WAVE per entry of X; then one
//                 workgroup per cut for its three P x Q sums.
//   k_brk_scores  one workgroup per record: BASE = the slabs left to right, the 8 (L - 1) scores (BASE + delta) /
//                 total, and the record's pick (pick_first_max_256, hicmi_internal.h) over the candidates of brk_counts.
// No candidate bin order is built.  Matrix reads per record: L (n - L) for X's rows (each re-read from cache for the
// L positions: L^2 (n - L) multiply-adds) and L^3 / 6 for the P x Q sums; the finishing kernel does 8 L^2 look-ups.
//
// LDS: neither kernel has dynamic LDS or stages anything whose size depends on a record - the arrangement, X and the
// P x Q sums are read from global memory (L2) - so a launch that mixes a scaffold of a few bins with one of thousands
// has no threshold to fall on either side of.
#include "hicmi_internal.h"

namespace hicmi {

// position inside the block of its bin t (as laid down in A) in candidate k of cut p
__device__ __forceinline__ int brk_newpos(int t, int p, int L, int k)
{
    const int w = k >> 2, x = (k >> 1) & 1, y = k & 1;
    if (t < p) return (w ? L - p : 0) + (x ? p - 1 - t : t);
    const int b = t - p, q = L - p;
    return (w ? 0 : p) + (y ? q - 1 - b : b);
}

// a candidate that competes: both pieces have min_piece bins, and its bin order differs from A's, from the in-place
// whole flip's and from every earlier candidate's of the same cut
__device__ __forceinline__ bool brk_counts(int p, int L, int k, int min_piece)
{
    const int q = L - p, x = (k >> 1) & 1, y = k & 1;
    if (p < min_piece || q < min_piece) return false;
    if ((x && p == 1) || (y && q == 1)) return false;   // reversing one bin: the candidate without that reversal came first
    if (k == 0 || k == 7) return false;                  // A, and the whole scaffold flipped in place
    if (k == 5 && p == 1) return false;                  // Q reversed in front of a one-bin P: the whole flip
    if (k == 6 && q == 1) return false;
    if (k == 4 && p == 1 && q == 1) return false;
    return true;
}

__global__ __launch_bounds__(256) void k_brk_tables(const BrkRec* __restrict__ recs, int n_rec)
{
    __shared__ double s_w[3][4];
    const int64_t bx0 = blockIdx.x;
    int lo = 0, hi = n_rec - 1;                          // the last record whose first workgroup is at or before this one
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (recs[mid].wg0 <= bx0) lo = mid; else hi = mid - 1;
    }
    const BrkRec& d = recs[lo];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int L = d.L, B = d.B, n = d.n;
    const int32_t* __restrict__ pos = d.pos;
    const double* __restrict__ H = d.H;
    int64_t bx = bx0 - d.wg0;
    if (bx < d.n_base) {
        base_partial_body(d.M2, d.ld2, pos, n, H, n, (int)bx, d.n_base, d.base + bx);
        return;
    }
    bx -= d.n_base;
    const int qb = (L + 3) >> 2;
    if (bx < (int64_t)L * qb) {
        const int t = (int)(bx / qb), q = (int)(bx - (int64_t)t * qb) * 4 + wave;
        if (q >= L) return;
        const double* __restrict__ row = d.M2 + (int64_t)pos[B + t] * d.ld2;
        const double hn = H[n - 1];
        const int at = B + q;
        double acc = 0.0;
#pragma unroll 4
        for (int o = lane; o < B; o += 64) acc += row[pos[o]] * (hn - H[at - o - 1]);
#pragma unroll 4
        for (int o = B + L + lane; o < n; o += 64) acc += row[pos[o]] * (hn - H[o - at - 1]);
        acc = wave_sum_s(acc);
        if (lane == 0) d.X[(int64_t)t * L + q] = acc;
        return;
    }
    bx -= (int64_t)L * qb;
    const int p = (int)bx + 1;
    if (p >= L) return;
    const int q = L - p, cnt = p * q;
    double g1 = 0.0, g2 = 0.0, g3 = 0.0;
    for (int idx = threadIdx.x; idx < cnt; idx += 256) {
        const int a = idx / q, b = idx - a * q;
        const double m = d.M2[(int64_t)pos[B + a] * d.ld2 + pos[B + p + b]];
        const int dd = p + b - a;
        const double h0 = H[dd - 1];                     // h(d') - h(d) = H[d - 1] - H[d' - 1]
        g1 += m * (h0 - H[L - dd - 1]);
        g2 += m * (h0 - H[L - 2 - a - b]);
        g3 += m * (h0 - H[a + b]);
    }
    g1 = block_sum_256(g1, s_w[0]);
    g2 = block_sum_256(g2, s_w[1]);
    g3 = block_sum_256(g3, s_w[2]);
    if (threadIdx.x == 0) {
        double* out = d.pq + 3 * (int64_t)(p - 1);
        out[0] = g1; out[1] = g2; out[2] = g3;
    }
}

__global__ __launch_bounds__(256) void k_brk_scores(const BrkRec* __restrict__ recs, double near_top)
{
    __shared__ double s_part[BRK_BASE_SLABS], s_base;
    const BrkRec& d = recs[blockIdx.x];
    const int tid = threadIdx.x, L = d.L, mp = d.min_piece;
    for (int i = tid; i < BRK_BASE_SLABS; i += 256) s_part[i] = d.base[i];
    __syncthreads();
    if (tid == 0) s_base = serial_sum_lds(s_part, 0, BRK_BASE_SLABS, 0.0);
    __syncthreads();
    const double base = s_base, total = d.total;
    const double* __restrict__ X = d.X;
    const int n_cand = 8 * (L - 1);
    for (int c = tid; c < n_cand; c += 256) {
        const int p = (c >> 3) + 1, k = c & 7;
        double delta = 0.0;
        if (k) {
#pragma unroll 4
            for (int t = 0; t < L; t++) {
                const double* __restrict__ xr = X + (int64_t)t * L;
                delta += xr[brk_newpos(t, p, L, k)] - xr[t];
            }
            const double* __restrict__ pq = d.pq + 3 * (int64_t)(p - 1);
            if (k == 3 || k == 4) delta += pq[0];
            else if (k == 1 || k == 6) delta += pq[1];
            else if (k == 2 || k == 5) delta += pq[2];
        }
        d.scores[c] = (base + delta) / total;
    }
    pick_first_max_256(tid, n_cand, d.scores, d.best, near_top, [=](int c) { return brk_counts((c >> 3) + 1, L, c & 7, mp); });
}

void launch_brk(const BrkRec* recs, int n_rec, int64_t n_wg, double near_top, hipStream_t s)
{
    hipLaunchKernelGGL(k_brk_tables, dim3((unsigned)n_wg), dim3(256), 0, s, recs, n_rec);
    hipLaunchKernelGGL(k_brk_scores, dim3(n_rec), dim3(256), 0, s, recs, near_top);
}

}  // namespace hicmi
