// k_part2_support.hip - placement support of a finished Part 2 ordering (hicmi_p2_support_multi).
//
// For every scaffold j of a chromosome's final arrangement A the objective of "A without j, j put back at gap g in
// orientation r" is wanted for all S gaps and both orientations: 2 S^2 candidates per chromosome.  Each (chromosome,
// left-out scaffold) pair is ONE insertion step in the sense of k_part2_search.hip,
//     score(j, g, r) * total = BASE_j - STRADDLE_j(g) + CROSS_j(g, r),
// over the arrangement "A without j" (n - L_j bins, S - 1 scaffolds) with scaffold j (L_j bins) as the new one, and the
// host builds one SupRec per pair for the whole genome: blockIdx.y = record, as with InsStep.  Two launches:
//   k_sup_fast    workgroups [0, NB): the BASE slabs (base_partial_body, the arrangement without j staged in LDS);
//                 then one WAVE per position u of "A without j": its row's share s(u) of the STRADDLE increment of its
//                 own scaffold; then one workgroup per (gap, orientation): CROSS, 4 waves over the bins of j.
//   k_sup_scores  one workgroup per record: BASE = the slabs left to right, STRADDLE = prefix over the scaffolds in
//                 position order, the 2 S scores divided by the chromosome's total, and the record's pick
//                 (pick_first_max_256, hicmi_internal.h) over the candidates of sup_counts.
// "A without j" is never written anywhere in global memory: position q of it is position q (q < P_j) or q + L_j of A,
// and its gap g starts at arr_pos[g] (g <= j) or arr_pos[g + 1] - L_j.  No candidate bin order is built either.
// Matrix reads per record: n^2/2 (BASE) + n^2 (rows) + 2 S L_j n (CROSS); summed over j that is (3/2 + 2) S n^2 per
// chromosome instead of the S^2 n^2 of scoring 2 S^2 materialised rows.
//
// LDS: k_sup_fast's dynamic LDS is 4 bytes per bin of the launch's LARGEST chromosome and every workgroup stages only
// its own n - L_j <= that; k_sup_scores holds S + 1 doubles (S <= SUP_MAX_S) and reads the row values from L2, so
// neither kernel has a staging threshold that a launch mixing small and large chromosomes could fall on either side of.
#include "hicmi_internal.h"

namespace hicmi {

// position q of "A without j" -> position of A
__device__ __forceinline__ int sup_skip(int q, int Pj, int L) { return q < Pj ? q : q + L; }
// start of gap g (0 ... S - 1) of "A without j"
__device__ __forceinline__ int sup_gap_pos(const int32_t* __restrict__ arr_pos, int g, int j, int L)
{
    return g <= j ? arr_pos[g] : arr_pos[g + 1] - L;
}

__global__ __launch_bounds__(256) void k_sup_fast(const SupRec* __restrict__ recs, int n_base_blocks, int n_row_blocks)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_w[4];
    const SupRec& d = recs[blockIdx.y];
    const int S = d.S, j = d.j, L = d.L, n_arr = d.n - d.L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* __restrict__ pos = d.pos;
    const int32_t* __restrict__ arr_pos = d.arr_pos;
    const double* __restrict__ H = d.H;
    const int Pj = arr_pos[j];
    int bx = blockIdx.x;
    if (bx < n_base_blocks) {
        int32_t* pl = reinterpret_cast<int32_t*>(smem);
        for (int q = threadIdx.x; q < n_arr; q += 256) pl[q] = pos[sup_skip(q, Pj, L)];
        __syncthreads();
        base_partial_body(d.M2, d.ld2, pl, n_arr, H, d.n, bx, n_base_blocks, d.partial + bx);
        return;
    }
    bx -= n_base_blocks;
    if (bx < n_row_blocks) {
        const int u = bx * 4 + wave;
        if (u >= n_arr) return;
        int below = 0;                                    // scaffold of position u: the last gap that starts at or before u
        for (int g = lane; g < S; g += 64) below += sup_gap_pos(arr_pos, g, j, L) <= u;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) below += __shfl_xor(below, off, 64);
        const int g = below - 1;
        const int P0 = sup_gap_pos(arr_pos, g, j, L), P1 = sup_gap_pos(arr_pos, g + 1, j, L);
        const double* __restrict__ row = d.M2 + (int64_t)pos[sup_skip(u, Pj, L)] * d.ld2;
        double acc = 0.0;
#pragma unroll 4
        for (int q = lane; q < P0; q += 64) {
            const int dd = u - q;
            acc -= row[pos[sup_skip(q, Pj, L)]] * (H[dd + L - 1] - H[dd - 1]);
        }
#pragma unroll 4
        for (int q = P1 + lane; q < n_arr; q += 64) {
            const int dd = q - u;
            acc += row[pos[sup_skip(q, Pj, L)]] * (H[dd + L - 1] - H[dd - 1]);
        }
        acc = wave_sum_s(acc);
        if (lane == 0) d.partial[n_base_blocks + u] = acc;
        return;
    }
    const int c = bx - n_row_blocks;
    if (c >= 2 * S) return;
    const int g = c >> 1, r = c & 1, P = sup_gap_pos(arr_pos, g, j, L);
    const double hn = H[d.n - 1];
    double acc = 0.0;
    for (int e = wave; e < L; e += 4) {
        const int xe = d.start + (r ? L - 1 - e : e);
        const double* __restrict__ row = d.M2 + (int64_t)xe * d.ld2;
#pragma unroll 4
        for (int q = lane; q < n_arr; q += 64) {
            const int dd = q < P ? (P + e - q) : (q + L - (P + e));
            acc += row[pos[sup_skip(q, Pj, L)]] * (hn - H[dd - 1]);
        }
        for (int e2 = e + 1 + lane; e2 < L; e2 += 64) {
            const int x2 = d.start + (r ? L - 1 - e2 : e2);
            acc += row[x2] * (hn - H[e2 - e - 1]);
        }
    }
    const double sum = block_sum_256(acc, s_w);
    if (threadIdx.x == 0) d.partial[n_base_blocks + n_arr + c] = sum;
}

// a candidate whose bin order differs from A's and that is not the second of two equal bin orders: not j's own gap
// in its own orientation; of a one-bin scaffold only '+' counts anywhere ('-' is the same bin order and comes second,
// so it can never be a strict maximum) and its own gap not at all.  A chromosome of one scaffold has no other
// placement: its flip is the whole chromosome read backwards.
__device__ __forceinline__ bool sup_counts(int i, int j, int L, int cur_rev, int S)
{
    const int g = i >> 1, r = i & 1;
    if (S == 1) return false;
    if (L == 1) return r == 0 && g != j;
    return !(g == j && r == cur_rev);
}

__global__ __launch_bounds__(256) void k_sup_scores(const SupRec* __restrict__ recs, int n_base_blocks, double near_top)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_s[];
    double* buf = reinterpret_cast<double*>(smem_s);     // the STRADDLE prefix, S + 1 entries
    __shared__ double s_part[SUP_BASE_SLABS], s_base;
    const SupRec& d = recs[blockIdx.x];
    const int tid = threadIdx.x, S = d.S, j = d.j, L = d.L, n_arr = d.n - d.L;
    const double* __restrict__ partial = d.partial;
    for (int i = tid; i < n_base_blocks; i += 256) s_part[i] = partial[i];
    // STRADDLE(g + 1) - STRADDLE(g): the rows of the scaffold after gap g, added in position order
    for (int g = tid; g < S - 1; g += 256) {
        const int P0 = sup_gap_pos(d.arr_pos, g, j, L), P1 = sup_gap_pos(d.arr_pos, g + 1, j, L);
        double acc = 0.0;
        for (int u = P0; u < P1; u++) acc += partial[n_base_blocks + u];
        buf[g + 1] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        s_base = serial_sum_lds(s_part, 0, n_base_blocks, 0.0);
        buf[0] = 0.0;
        serial_prefix_lds(buf, 1, S, 0.0);
    }
    __syncthreads();
    const double base = s_base, total = d.total;
    const double* __restrict__ cross = partial + n_base_blocks + n_arr;
    const int n_cand = 2 * S, cur_rev = d.cur_rev;
    for (int i = tid; i < n_cand; i += 256) d.scores[i] = (base - buf[i >> 1] + cross[i]) / total;
    pick_first_max_256(tid, n_cand, d.scores, d.best, near_top, [=](int i) { return sup_counts(i, j, L, cur_rev, S); });
}

static std::atomic<int> g_lds_sup_fast{0}, g_lds_sup_scores{0};

void launch_sup(const SupRec* recs, int n_rec, int max_S, int max_n, double near_top, hipStream_t s)
{
    const int NB = SUP_BASE_SLABS, n_row_blocks = (max_n + 3) / 4, n_cross_blocks = 2 * max_S;
    const size_t lds = (((size_t)max_n * sizeof(int32_t)) + 15) & ~(size_t)15;
    const size_t lds2 = (((size_t)(max_S + 1) * sizeof(double)) + 15) & ~(size_t)15;
    ensure_dynamic_lds(reinterpret_cast<const void*>(k_sup_fast), g_lds_sup_fast, lds);
    ensure_dynamic_lds(reinterpret_cast<const void*>(k_sup_scores), g_lds_sup_scores, lds2);
    for (int r0 = 0; r0 < n_rec; r0 += 65535) {           // blockIdx.y = record
        const int cnt = n_rec - r0 < 65535 ? n_rec - r0 : 65535;
        hipLaunchKernelGGL(k_sup_fast, dim3(NB + n_row_blocks + n_cross_blocks, cnt), dim3(256), lds, s, recs + r0, NB,
                           n_row_blocks);
        hipLaunchKernelGGL(k_sup_scores, dim3(cnt), dim3(256), lds2, s, recs + r0, NB, near_top);
    }
}

}  // namespace hicmi
