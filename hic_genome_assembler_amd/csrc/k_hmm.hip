// k_hmm.hip - the 2-state diagonal Gaussian HMM boundary finder (S2C:730-942, hmm = True) on gfx950, fp64.
//
// The observations X (T x D, row-major, leading dimension ld) are one contiguous buffer owned by the context.  Every
// pass over X is one of two shapes:
//   * row pass: one wave per row, lanes stride over the columns and reduce with shuffles (emission dot products,
//     k-means distances);
//   * column pass: a workgroup owns 256 consecutive columns of a chunk of rows, every thread sums its column over the
//     chunk; the per-chunk partials are combined in a fixed order by a second kernel (column statistics, k-means
//     center sums, the M-step's gamma^T X and gamma^T X^2).
// The forward / backward recursion and Viterbi are chunked scans of 2 x 2 matrices in the (logsumexp, +) and (max, +)
// semirings, run by one workgroup.  Every reduction has a fixed order, so a run is reproducible.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "hicmi_internal.h"

namespace hicmi {

static constexpr double kLn10 = 2.302585092994046;         // math.log(10), the divisor of modularity.log_transform
static constexpr int kColThreads = 256;
static constexpr int kScanThreads = 512;

int hmm_col_chunks(int T, int D)
{
    const int col_blocks = (D + kColThreads - 1) / kColThreads;
    int r = (2048 + col_blocks - 1) / col_blocks;
    if (r > 1024) r = 1024;
    if (r > T) r = T;
    return r < 1 ? 1 : r;
}

// ---- observation build: X[t][d] = log10(sim + 1) (0 where sim == 0) of rows / columns c + t, c + d in `order`
__device__ __forceinline__ double hmm_similarity(double c, double sig, double rs)
{
    double d = (1.0 - (c / sig)) + 1.0;                       // the cell of k_sort.hip's similarity(), S2C:147-149
    return rs * (1.0 - (d - 1.0));
}

__global__ __launch_bounds__(256) void k_hmm_obs(const double* __restrict__ C, int64_t ldc, const int32_t* __restrict__ order,
                                                 const double* __restrict__ np_sum, const double* __restrict__ seq_sum,
                                                 int c, int T, int D, double* __restrict__ X)
{
    const int t = blockIdx.y;
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (t >= T || d >= D) return;
    const int pa = order[c + t];
    const double s = hmm_similarity(C[(int64_t)pa * ldc + order[c + d]], np_sum[pa], seq_sum[pa]);
    X[(int64_t)t * D + d] = s != 0.0 ? log(s + 1.0) / kLn10 : 0.0;
}

void launch_hmm_obs(const double* C, int64_t ldc, const int32_t* order, const double* np_sum, const double* seq_sum,
                    int c, int T, int D, double* X, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_obs, dim3((D + 255) / 256, T), dim3(256), 0, s, C, ldc, order, np_sum, seq_sum, c, T, D, X);
}

// ---- column pass: partial sums per (row chunk, column).  mode 0: (x - shift), (x - shift)^2; mode 1: x where
// label == 0, x where label == 1; mode 2: g0 x, g1 x, g0 x^2, g1 x^2 (g = posteriors, T x 2).  Column d of row chunk
// `chunk` (rows [chunk * rows_per, min(T, (chunk + 1) * rows_per))), written to part[chunk][q][d].
template <int MODE>
__device__ __forceinline__ void colsum_chunk(const double* __restrict__ X, int64_t ld, int T, int D, int rows_per, int chunk,
                                             int d, const double* __restrict__ shift, const int32_t* __restrict__ labels,
                                             const double* __restrict__ g, double* __restrict__ part)
{
    const int t0 = chunk * rows_per;
    const int t1 = min(T, t0 + rows_per);
    constexpr int NQ = MODE == 2 ? 4 : 2;
    double s[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) s[q] = 0.0;
    const double sh = (MODE == 0 && shift) ? shift[d] : 0.0;
    for (int t = t0; t < t1; t++) {
        const double x = X[(int64_t)t * ld + d];
        if constexpr (MODE == 0) {
            const double v = x - sh;
            s[0] += v;
            s[1] += v * v;
        } else if constexpr (MODE == 1) {
            if (labels[t]) s[1] += x; else s[0] += x;
        } else {
            const double g0 = g[2 * t], g1 = g[2 * t + 1], x2 = x * x;
            s[0] += g0 * x;
            s[1] += g1 * x;
            s[2] += g0 * x2;
            s[3] += g1 * x2;
        }
    }
#pragma unroll
    for (int q = 0; q < NQ; q++) part[((int64_t)chunk * NQ + q) * D + d] = s[q];
}

template <int MODE>
__global__ __launch_bounds__(256) void k_hmm_colsum(const double* __restrict__ X, int64_t ld, int T, int D, int rows_per,
                                                    const double* __restrict__ shift, const int32_t* __restrict__ labels,
                                                    const double* __restrict__ g, double* __restrict__ part)
{
    const int d = blockIdx.x * kColThreads + threadIdx.x;
    if (d >= D) return;
    colsum_chunk<MODE>(X, ld, T, D, rows_per, blockIdx.y, d, shift, labels, g, part);
}

// out[i] = sum over chunks (in chunk order) of part[chunk][i], i < NQ * D
__device__ __forceinline__ double combine_one(const double* __restrict__ part, int R, int NQ, int D, int i)
{
    double s = 0.0;
    for (int r = 0; r < R; r++) s += part[(int64_t)r * NQ * D + i];
    return s;
}

__global__ __launch_bounds__(256) void k_hmm_combine(const double* __restrict__ part, int R, int NQ, int D,
                                                     double* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= NQ * D) return;
    out[i] = combine_one(part, R, NQ, D, i);
}

void launch_hmm_colsum(int mode, const double* X, int64_t ld, int T, int D, const double* shift, const int32_t* labels,
                       const double* g, double* part, double* out, hipStream_t s)
{
    int rows_per, Rr;                                         // Rr: chunks that hold rows
    hmm_col_shape(T, hmm_col_chunks(T, D), rows_per, Rr);
    const dim3 grid((D + kColThreads - 1) / kColThreads, Rr);
    const int nq = mode == 2 ? 4 : 2;
    if (mode == 0) hipLaunchKernelGGL(k_hmm_colsum<0>, grid, dim3(kColThreads), 0, s, X, ld, T, D, rows_per, shift, labels, g, part);
    else if (mode == 1) hipLaunchKernelGGL(k_hmm_colsum<1>, grid, dim3(kColThreads), 0, s, X, ld, T, D, rows_per, shift, labels, g, part);
    else hipLaunchKernelGGL(k_hmm_colsum<2>, grid, dim3(kColThreads), 0, s, X, ld, T, D, rows_per, shift, labels, g, part);
    hipLaunchKernelGGL(k_hmm_combine, dim3((nq * D + 255) / 256), dim3(256), 0, s, part, Rr, nq, D, out);
}

// ---- row pass helpers
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// sum_d (x[d] - cen[k][d])^2 for k < nc (nc = 1 or 2), reduced over the wave: the distances of one row
__device__ __forceinline__ void dist2_row(const double* __restrict__ x, int D, const double* __restrict__ cen, int nc, int lane,
                                          double& a0, double& a1)
{
    a0 = 0.0; a1 = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = x[d];
        const double e0 = v - cen[d];
        a0 += e0 * e0;
        if (nc > 1) { const double e1 = v - cen[D + d]; a1 += e1 * e1; }
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
}

// dist[k][t] = sum_d (X[t][d] - cen[k][d])^2 for k < nc (nc = 1 or 2)
__global__ __launch_bounds__(256) void k_hmm_dist2(const double* __restrict__ X, int64_t ld, int T, int D,
                                                   const double* __restrict__ cen, int nc, double* __restrict__ dist)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    double a0, a1;
    dist2_row(X + (int64_t)t * ld, D, cen, nc, lane, a0, a1);
    if (lane == 0) {
        dist[t] = a0;
        if (nc > 1) dist[T + t] = a1;
    }
}

void launch_hmm_dist2(const double* X, int64_t ld, int T, int D, const double* cen, int nc, double* dist, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_dist2, dim3((T + 3) / 4), dim3(256), 0, s, X, ld, T, D, cen, nc, dist);
}

// ---- k-means: assignment (ties to center 0, as sklearn's strict '<'), plus the counters of the iteration
// st: [0] rows whose label changed, [1] rows with label 1
__device__ __forceinline__ void assign_row(const double* __restrict__ x, int D, const double* __restrict__ cen, int lane,
                                           int t, const int32_t* __restrict__ old_labels, int32_t* __restrict__ labels,
                                           double* __restrict__ mind, int* __restrict__ changed, int* __restrict__ n1)
{
    double a0 = 0.0, a1 = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = x[d];
        const double e0 = v - cen[d], e1 = v - cen[D + d];
        a0 += e0 * e0;
        a1 += e1 * e1;
    }
    a0 = wave_sum(a0);
    a1 = wave_sum(a1);
    if (lane == 0) {
        const int l = a1 < a0 ? 1 : 0;
        labels[t] = l;
        mind[t] = l ? a1 : a0;
        if (l != old_labels[t]) atomicAdd(changed, 1);
        if (l) atomicAdd(n1, 1);
    }
}

__global__ __launch_bounds__(256) void k_hmm_assign(const double* __restrict__ X, int64_t ld, int T, int D,
                                                    const double* __restrict__ cen, const int32_t* __restrict__ old_labels,
                                                    int32_t* __restrict__ labels, double* __restrict__ mind,
                                                    int* __restrict__ st)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    assign_row(X + (int64_t)t * ld, D, cen, lane, t, old_labels, labels, mind, &st[0], &st[1]);
}

// new centers from the combined sums (an empty cluster keeps its center); returns the summed squared shift in thread 0.
// red: 1024 doubles of LDS, blockDim.x == 1024
__device__ __forceinline__ double center_update_block(const double* __restrict__ sums, int T, int D, int n1,
                                                      double* __restrict__ cen, double* red)
{
    const int n0 = T - n1;
    double sh = 0.0;
    for (int i = threadIdx.x; i < 2 * D; i += 1024) {
        const int k = i / D;
        const int cnt = k ? n1 : n0;
        const double old = cen[i];
        const double nw = cnt > 0 ? sums[i] / (double)cnt : old;
        const double e = nw - old;
        sh += e * e;
        cen[i] = nw;
    }
    red[threadIdx.x] = sh;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// sum of v[0..n) in a fixed order (returned in thread 0); red: 1024 doubles of LDS, blockDim.x == 1024
__device__ __forceinline__ double sum_block(const double* __restrict__ v, int n, double* red)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) s += v[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// out[0] = sum_d of the squared shift, out[2], out[3] = the iteration's counters (one read-back per Lloyd iteration)
__global__ __launch_bounds__(1024) void k_hmm_center_update(const double* __restrict__ sums, int T, int D,
                                                            const int* __restrict__ st, double* __restrict__ cen,
                                                            double* __restrict__ shift_out)
{
    __shared__ double red[1024];
    const double sh = center_update_block(sums, T, D, st[1], cen, red);
    if (threadIdx.x == 0) {
        shift_out[0] = sh;
        shift_out[2] = (double)st[0];
        shift_out[3] = (double)st[1];
    }
}

__global__ __launch_bounds__(1024) void k_hmm_sum(const double* __restrict__ v, int n, double* __restrict__ out)
{
    __shared__ double red[1024];
    const double s = sum_block(v, n, red);
    if (threadIdx.x == 0) *out = s;
}

void launch_hmm_assign(const double* X, int64_t ld, int T, int D, const double* cen, const int32_t* old_labels,
                       int32_t* labels, double* mind, int* st, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_assign, dim3((T + 3) / 4), dim3(256), 0, s, X, ld, T, D, cen, old_labels, labels, mind, st);
}

void launch_hmm_center_update(const double* sums, int T, int D, const int* st, double* cen, double* shift_out, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_center_update, dim3(1), dim3(1024), 0, s, sums, T, D, st, cen, shift_out);
}

void launch_hmm_sum(const double* v, int n, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_sum, dim3(1), dim3(1024), 0, s, v, n, out);
}

// ---- model parameters on the device (HmmParams offsets into one fp64 buffer, see hicmi_internal.h)
// per column: mean / covar of both states (from the M-step sums, or as given), and the emission operands
__global__ __launch_bounds__(256) void k_hmm_mstep_cols(const double* __restrict__ sums, const double* __restrict__ post,
                                                        int D, int from_sums, double* __restrict__ P)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * D) return;
    const int k = i / D;
    double* mean = P + HMM_P_MEAN * (int64_t)D;
    double* var = P + HMM_P_VAR * (int64_t)D;
    if (from_sums) {
        // hmmlearn GaussianHMM._do_mstep, diag: means_prior 0, means_weight 0, covars_prior 1e-2, covars_weight 1
        const double pk = post[k];
        const double obs = sums[i], obs2 = sums[2 * D + i];
        const double mu = obs / pk;
        const double cn = ((obs2 - 2.0 * mu * obs) + mu * mu * pk);
        mean[i] = mu;
        var[i] = (1e-2 + cn) / fmax(pk, 1e-5);
    }
    const double mu = mean[i], v = var[i];
    P[HMM_P_MOV * (int64_t)D + i] = mu / v;
    P[HMM_P_IV * (int64_t)D + i] = 1.0 / v;
    P[HMM_P_LOGV * (int64_t)D + i] = log(v);
    P[HMM_P_MU2V * (int64_t)D + i] = (mu * mu) / v;
}

// the emission constants of both states and, after an E-step, the new transition matrix
// (normalize_rows(where(A == 0, 0, xi)), a zero row left as it is)
__global__ __launch_bounds__(1024) void k_hmm_mstep_final(int D, int update_trans, double* __restrict__ P)
{
    __shared__ double red[4][1024];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const double* logv = P + HMM_P_LOGV * (int64_t)D;
    const double* mu2v = P + HMM_P_MU2V * (int64_t)D;
    for (int d = threadIdx.x; d < D; d += 1024) {
        s[0] += logv[d];
        s[1] += logv[D + d];
        s[2] += mu2v[d];
        s[3] += mu2v[D + d];
    }
    for (int q = 0; q < 4; q++) red[q][threadIdx.x] = s[q];
    __syncthreads();
    for (int w = 512; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int q = 0; q < 4; q++) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double* sc = P + HMM_P_SCALARS * (int64_t)D;
    const double base = (double)D * log(2.0 * M_PI);
    sc[HMM_S_CONST + 0] = (base + red[0][0]) + red[2][0];
    sc[HMM_S_CONST + 1] = (base + red[1][0]) + red[3][0];
    if (update_trans) {
        for (int i = 0; i < 2; i++) {
            double a[2];
            for (int j = 0; j < 2; j++) a[j] = sc[HMM_S_A + 2 * i + j] == 0.0 ? 0.0 : fmax(sc[HMM_S_XI + 2 * i + j], 0.0);
            double rs = a[0] + a[1];
            if (rs == 0.0) rs = 1.0;
            for (int j = 0; j < 2; j++) sc[HMM_S_A + 2 * i + j] = a[j] / rs;
        }
    }
    for (int q = 0; q < 4; q++) sc[HMM_S_LOGA + q] = log(sc[HMM_S_A + q]);
    for (int q = 0; q < 2; q++) sc[HMM_S_LOGPI + q] = log(sc[HMM_S_PI + q]);
}

void launch_hmm_params(const double* sums, int D, int from_sums, double* P, hipStream_t s)
{
    const double* post = P + HMM_P_SCALARS * (int64_t)D + HMM_S_POST;
    hipLaunchKernelGGL(k_hmm_mstep_cols, dim3((2 * D + 255) / 256), dim3(256), 0, s, sums, post, D, from_sums, P);
    hipLaunchKernelGGL(k_hmm_mstep_final, dim3(1), dim3(1024), 0, s, D, from_sums, P);
}

// ---- emission: L[t][k] = -0.5 (const_k - 2 x.(mu_k/var_k) + x^2.(1/var_k)), one wave per row
__global__ __launch_bounds__(256) void k_hmm_emission(const double* __restrict__ X, int64_t ld, int T, int D,
                                                      const double* __restrict__ P, double* __restrict__ L)
{
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    const double* x = X + (int64_t)t * ld;
    const double* mov = P + HMM_P_MOV * (int64_t)D;
    const double* iv = P + HMM_P_IV * (int64_t)D;
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    for (int d = lane; d < D; d += 64) {
        const double v = x[d], v2 = v * v;
        a0 += v * mov[d];
        a1 += v * mov[D + d];
        b0 += v2 * iv[d];
        b1 += v2 * iv[D + d];
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); b0 = wave_sum(b0); b1 = wave_sum(b1);
    if (lane == 0) {
        const double* sc = P + HMM_P_SCALARS * (int64_t)D;
        L[2 * t] = -0.5 * ((sc[HMM_S_CONST] - 2.0 * a0) + b0);
        L[2 * t + 1] = -0.5 * ((sc[HMM_S_CONST + 1] - 2.0 * a1) + b1);
    }
}

void launch_hmm_emission(const double* X, int64_t ld, int T, int D, const double* P, double* L, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_emission, dim3((T + 3) / 4), dim3(256), 0, s, X, ld, T, D, P, L);
}

// ---- semirings over 2 x 2 matrices: (logsumexp, +) and (max, +)
template <bool MAX>
__device__ __forceinline__ double sr_add(double a, double b)
{
    if constexpr (MAX) return a > b ? a : b;
    else {
        if (a < b) { const double t = a; a = b; b = t; }
        if (b == -INFINITY) return a;
        return a + log1p(exp(b - a));
    }
}

struct M2 { double m[4]; };                                 // row-major [i][j]

template <bool MAX>
__device__ __forceinline__ M2 sr_mul(const M2& a, const M2& b)
{
    M2 c;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) c.m[2 * i + j] = sr_add<MAX>(a.m[2 * i] + b.m[j], a.m[2 * i + 1] + b.m[2 + j]);
    return c;
}

__device__ __forceinline__ M2 sr_identity()
{
    M2 c;
    c.m[0] = 0.0; c.m[1] = -INFINITY; c.m[2] = -INFINITY; c.m[3] = 0.0;
    return c;
}

// M_t[i][j] = logA[i][j] + L_t[j]
__device__ __forceinline__ M2 step_matrix(const double* logA, const double* __restrict__ L, int t)
{
    M2 c;
    const double l0 = L[2 * t], l1 = L[2 * t + 1];
    c.m[0] = logA[0] + l0; c.m[1] = logA[1] + l1; c.m[2] = logA[2] + l0; c.m[3] = logA[3] + l1;
    return c;
}

// inclusive scan of one M2 per thread in LDS (Hillis-Steele), forward (prefix) or backward (suffix)
template <bool MAX, bool SUFFIX>
__device__ __forceinline__ void block_scan(M2* s, M2 v)
{
    const int k = threadIdx.x;
    s[k] = v;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        M2 r = s[k];
        if (!SUFFIX && k >= off) r = sr_mul<MAX>(s[k - off], r);
        if (SUFFIX && k + off < kScanThreads) r = sr_mul<MAX>(r, s[k + off]);
        __syncthreads();
        s[k] = r;
        __syncthreads();
    }
}

// Forward, backward, posteriors, expected transitions and state occupancies of one E-step (one workgroup).
// Chunk k of S = ceil(T / 512) steps: the thread composes the M_t of its chunk, the chunk products are scanned both
// ways, then the thread walks its chunk from the scanned boundary values.  Writes alpha / beta / gamma (T x 2),
// logprob to hist[it] and xi / post into the scalar block of P.
__global__ __launch_bounds__(kScanThreads) void k_hmm_fb(const double* __restrict__ L, int T, double* __restrict__ P, int D,
                                                         double* __restrict__ alpha, double* __restrict__ beta,
                                                         double* __restrict__ gam, double* __restrict__ hist, int it)
{
    __shared__ M2 pre[kScanThreads];
    __shared__ M2 suf[kScanThreads];
    __shared__ double red[6][kScanThreads];
    __shared__ double s_logprob;
    double* sc = P + HMM_P_SCALARS * (int64_t)D;
    double logA[4];
#pragma unroll
    for (int q = 0; q < 4; q++) logA[q] = sc[HMM_S_LOGA + q];
    const int k = threadIdx.x;
    const int S = (T + kScanThreads - 1) / kScanThreads;
    const int t0 = min(T, k * S), t1 = min(T, t0 + S);

    M2 p = sr_identity();
    for (int t = max(t0, 1); t < t1; t++) p = sr_mul<false>(p, step_matrix(logA, L, t));
    block_scan<false, false>(pre, p);
    const M2 mine_pre = k > 0 ? pre[k - 1] : sr_identity();
    __syncthreads();
    block_scan<false, true>(suf, p);

    if (t0 < t1) {
        // forward: alpha_t[j] = logsumexp_i(alpha_{t-1}[i] + logA[i][j]) + L_t[j]
        double a0 = sc[HMM_S_LOGPI] + L[0], a1 = sc[HMM_S_LOGPI + 1] + L[1];
        int t = 1;
        if (k > 0) {
            const double b0 = sr_add<false>(a0 + mine_pre.m[0], a1 + mine_pre.m[2]);
            const double b1 = sr_add<false>(a0 + mine_pre.m[1], a1 + mine_pre.m[3]);
            a0 = b0; a1 = b1;
            t = t0;
        } else {
            alpha[0] = a0; alpha[1] = a1;
        }
        for (; t < t1; t++) {
            const double n0 = sr_add<false>(a0 + logA[0], a1 + logA[2]) + L[2 * t];
            const double n1 = sr_add<false>(a0 + logA[1], a1 + logA[3]) + L[2 * t + 1];
            a0 = n0; a1 = n1;
            alpha[2 * t] = a0; alpha[2 * t + 1] = a1;
        }
        if (t1 == T) s_logprob = sr_add<false>(a0, a1);
        // backward: beta_{T-1} = 0, beta_t[i] = logsumexp_j(logA[i][j] + L_{t+1}[j] + beta_{t+1}[j])
        double c0 = 0.0, c1 = 0.0;
        if (t1 < T && k + 1 < kScanThreads) {
            const M2& r = suf[k + 1];
            c0 = sr_add<false>(r.m[0], r.m[1]);
            c1 = sr_add<false>(r.m[2], r.m[3]);
        }
        beta[2 * (t1 - 1)] = c0; beta[2 * (t1 - 1) + 1] = c1;
        for (int u = t1 - 2; u >= t0; u--) {
            const double l0 = L[2 * (u + 1)], l1 = L[2 * (u + 1) + 1];
            const double n0 = sr_add<false>((logA[0] + l0) + c0, (logA[1] + l1) + c1);
            const double n1 = sr_add<false>((logA[2] + l0) + c0, (logA[3] + l1) + c1);
            c0 = n0; c1 = n1;
            beta[2 * u] = c0; beta[2 * u + 1] = c1;
        }
    }
    __threadfence_block();
    __syncthreads();
    const double logprob = s_logprob;
    double g0s = 0.0, g1s = 0.0;
    double xi[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int t = t0; t < t1; t++) {
        const double a0 = alpha[2 * t], a1 = alpha[2 * t + 1];
        const double h0 = a0 + beta[2 * t], h1 = a1 + beta[2 * t + 1];
        const double nrm = sr_add<false>(h0, h1);
        const double g0 = exp(h0 - nrm), g1 = exp(h1 - nrm);
        gam[2 * t] = g0; gam[2 * t + 1] = g1;
        g0s += g0; g1s += g1;
        if (t + 1 < T) {
            const double l0 = L[2 * (t + 1)], l1 = L[2 * (t + 1) + 1];
            const double e0 = beta[2 * (t + 1)], e1 = beta[2 * (t + 1) + 1];
            xi[0] = sr_add<false>(xi[0], (((a0 + logA[0]) + l0) + e0) - logprob);
            xi[1] = sr_add<false>(xi[1], (((a0 + logA[1]) + l1) + e1) - logprob);
            xi[2] = sr_add<false>(xi[2], (((a1 + logA[2]) + l0) + e0) - logprob);
            xi[3] = sr_add<false>(xi[3], (((a1 + logA[3]) + l1) + e1) - logprob);
        }
    }
    red[0][k] = g0s; red[1][k] = g1s;
    for (int q = 0; q < 4; q++) red[2 + q][k] = xi[q];
    __syncthreads();
    for (int w = kScanThreads / 2; w >= 1; w >>= 1) {
        if (k < w) {
            red[0][k] += red[0][k + w];
            red[1][k] += red[1][k + w];
            for (int q = 0; q < 4; q++) red[2 + q][k] = sr_add<false>(red[2 + q][k], red[2 + q][k + w]);
        }
        __syncthreads();
    }
    if (k == 0) {
        sc[HMM_S_POST] = red[0][0];
        sc[HMM_S_POST + 1] = red[1][0];
        for (int q = 0; q < 4; q++) sc[HMM_S_XI + q] = T > 1 ? exp(red[2 + q][0]) : 0.0;
        hist[it] = logprob;
    }
}

void launch_hmm_fb(const double* L, int T, double* P, int D, double* alpha, double* beta, double* gam, double* hist, int it,
                   hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_fb, dim3(1), dim3(kScanThreads), 0, s, L, T, P, D, alpha, beta, gam, hist, it);
}

// ---- Viterbi: delta by the (max, +) scan; the backtrack s_t = b_t(s_{t+1}), b_t(j) = argmax_i(delta_t[i] + logA[i][j])
// (ties to state 0), as a suffix scan of composed {0,1} -> {0,1} maps.  A map is 2 bits: bit j = image of j.
__device__ __forceinline__ int map_compose(int f, int g)        // f o g
{
    return ((f >> (g & 1)) & 1) | (((f >> ((g >> 1) & 1)) & 1) << 1);
}

__global__ __launch_bounds__(kScanThreads) void k_hmm_viterbi(const double* __restrict__ L, int T, const double* __restrict__ P,
                                                              int D, uint8_t* __restrict__ bt, int32_t* __restrict__ states)
{
    __shared__ M2 pre[kScanThreads];
    __shared__ int maps[kScanThreads];
    __shared__ int s_last;
    const double* sc = P + HMM_P_SCALARS * (int64_t)D;
    double logA[4];
#pragma unroll
    for (int q = 0; q < 4; q++) logA[q] = sc[HMM_S_LOGA + q];
    const int k = threadIdx.x;
    const int S = (T + kScanThreads - 1) / kScanThreads;
    const int t0 = min(T, k * S), t1 = min(T, t0 + S);

    M2 p = sr_identity();
    for (int t = max(t0, 1); t < t1; t++) p = sr_mul<true>(p, step_matrix(logA, L, t));
    block_scan<true, false>(pre, p);
    const M2 mine_pre = k > 0 ? pre[k - 1] : sr_identity();

    int g = 2;                                                  // identity map
    if (t0 < t1) {
        double a0 = sc[HMM_S_LOGPI] + L[0], a1 = sc[HMM_S_LOGPI + 1] + L[1];
        if (k > 0) {
            const double b0 = fmax(a0 + mine_pre.m[0], a1 + mine_pre.m[2]);
            const double b1 = fmax(a0 + mine_pre.m[1], a1 + mine_pre.m[3]);
            a0 = b0; a1 = b1;                                  // delta_{t0 - 1}
        }
        for (int t = (k > 0 ? t0 : 1); t <= t1; t++) {
            // a = delta_{t-1}: its back-pointer map b_{t-1}, then (t < t1) delta_t
            const int u = t - 1;
            if (u >= t0 && u + 1 < T) {
                const int b0 = (a1 + logA[2] > a0 + logA[0]) ? 1 : 0;
                const int b1 = (a1 + logA[3] > a0 + logA[1]) ? 1 : 0;
                const int m = b0 | (b1 << 1);
                bt[u] = (uint8_t)m;
                g = map_compose(g, m);
            }
            if (u == T - 1) s_last = a1 > a0 ? 1 : 0;
            if (t < t1) {
                const double n0 = fmax(a0 + logA[0], a1 + logA[2]) + L[2 * t];
                const double n1 = fmax(a0 + logA[1], a1 + logA[3]) + L[2 * t + 1];
                a0 = n0; a1 = n1;
            }
        }
    }
    // suffix scan of the chunk maps: H_k = G_k o G_{k+1} o ...
    maps[k] = g;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        int r = maps[k];
        if (k + off < kScanThreads) r = map_compose(r, maps[k + off]);
        __syncthreads();
        maps[k] = r;
        __syncthreads();
    }
    __threadfence_block();
    if (t0 < t1) {
        const int last = s_last;
        int st = (t1 < T && k + 1 < kScanThreads) ? ((maps[k + 1] >> last) & 1) : last;   // s_{t1}, or s_{T-1}
        int u = t1 - 1;
        if (t1 == T) { states[T - 1] = last; u = T - 2; }
        for (; u >= t0; u--) {
            st = (bt[u] >> st) & 1;
            states[u] = st;
        }
    }
}

void launch_hmm_viterbi(const double* L, int T, const double* P, int D, uint8_t* bt, int32_t* states, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_viterbi, dim3(1), dim3(kScanThreads), 0, s, L, T, P, D, bt, states);
}

// ---- many k-means problems in lock step (hicmi_hmm_dist2_multi / hicmi_hmm_kmeans_multi).  Problem p is one
// workgroup row of the grid (blockIdx.y); its workgroups walk their rows / column chunks grid-stride and run the device
// functions of the single-problem kernels above with that problem's own chunking, so every result equals the single
// call's bit for bit.  A finished problem's workgroups return at once.
__global__ __launch_bounds__(256) void k_hmm_multi_seed(const HmmKmProb* __restrict__ pr, HmmKmState* __restrict__ st,
                                                        int kmeans)
{
    const HmmKmProb& q = pr[blockIdx.y];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < q.nc * q.D; i += gridDim.x * 256) {
        const int k = i / q.D, d = i - k * q.D;
        q.cen[i] = q.X[q.rows[k] * q.ld + d];
    }
    if (!kmeans) return;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < q.T; t += gridDim.x * 256) q.lab[t] = -1;     // "no label yet"
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        HmmKmState& s = st[blockIdx.y];
        s.phase = HMM_KM_LLOYD; s.cur = 0; s.it = 0; s.strict = 0; s.changed = 0; s.n1 = 0; s.inertia = 0.0;
    }
}

__global__ __launch_bounds__(256) void k_hmm_dist2_multi(const HmmKmProb* __restrict__ pr)
{
    const HmmKmProb& q = pr[blockIdx.y];
    const int lane = threadIdx.x & 63;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < q.T; t += gridDim.x * 4) {
        double a0, a1;
        dist2_row(q.X + (int64_t)t * q.ld, q.D, q.cen, q.nc, lane, a0, a1);
        if (lane == 0) {
            q.out[t] = a0;
            if (q.nc > 1) q.out[q.T + t] = a1;
        }
    }
}

// assignment of the live problems: Lloyd iterations and the final labels from the final centers
__global__ __launch_bounds__(256) void k_hmm_assign_multi(const HmmKmProb* __restrict__ pr, HmmKmState* __restrict__ st)
{
    HmmKmState& s = st[blockIdx.y];
    const int phase = s.phase;
    if (phase != HMM_KM_LLOYD && phase != HMM_KM_FINAL) return;
    const HmmKmProb& q = pr[blockIdx.y];
    const int cur = s.cur;
    const int32_t* old_labels = q.lab + (int64_t)cur * q.T;
    int32_t* labels = q.lab + (int64_t)(cur ^ 1) * q.T;
    const int lane = threadIdx.x & 63;
    for (int t = blockIdx.x * 4 + (threadIdx.x >> 6); t < q.T; t += gridDim.x * 4)
        assign_row(q.X + (int64_t)t * q.ld, q.D, q.cen, lane, t, old_labels, labels, q.out, &s.changed, &s.n1);
}

// label-masked column sums of the problems in a Lloyd iteration: work items (row chunk, 256 columns)
__global__ __launch_bounds__(256) void k_hmm_colsum_multi(const HmmKmProb* __restrict__ pr, const HmmKmState* __restrict__ st)
{
    const HmmKmState& s = st[blockIdx.y];
    if (s.phase != HMM_KM_LLOYD) return;
    const HmmKmProb& q = pr[blockIdx.y];
    const int32_t* labels = q.lab + (int64_t)(s.cur ^ 1) * q.T;
    const int cb = (q.D + kColThreads - 1) / kColThreads;
    for (int item = blockIdx.x; item < q.Rr * cb; item += gridDim.x) {
        const int chunk = item / cb;
        const int d = (item - chunk * cb) * kColThreads + threadIdx.x;
        if (d < q.D) colsum_chunk<1>(q.X, q.ld, q.T, q.D, q.rows_per, chunk, d, nullptr, labels, nullptr, q.part);
    }
}

__global__ __launch_bounds__(256) void k_hmm_combine_multi(const HmmKmProb* __restrict__ pr, const HmmKmState* __restrict__ st)
{
    if (st[blockIdx.y].phase != HMM_KM_LLOYD) return;
    const HmmKmProb& q = pr[blockIdx.y];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * q.D; i += gridDim.x * 256) q.sums[i] = combine_one(q.part, q.Rr, 2, q.D, i);
}

// one workgroup per problem: the center update and sklearn's stop rule (strict convergence when no label changed, else
// squared center shift <= tol, else max_iter), then - once the final labels are in - the inertia
__global__ __launch_bounds__(1024) void k_hmm_step_multi(const HmmKmProb* __restrict__ pr, HmmKmState* __restrict__ st,
                                                         int* __restrict__ done)
{
    __shared__ double red[1024];
    __shared__ int s_next;
    HmmKmState& s = st[blockIdx.x];
    const int phase = s.phase;
    if (phase != HMM_KM_LLOYD && phase != HMM_KM_FINAL) return;
    const HmmKmProb& q = pr[blockIdx.x];
    if (phase == HMM_KM_LLOYD) {
        const double sh = center_update_block(q.sums, q.T, q.D, s.n1, q.cen, red);
        if (threadIdx.x == 0) {
            s.cur ^= 1;
            s.it++;
            int next = HMM_KM_LLOYD;
            if (s.changed == 0) { s.strict = 1; next = HMM_KM_SUM; }
            else if (sh <= q.tol || s.it >= q.max_iter) next = HMM_KM_FINAL;
            s.changed = 0; s.n1 = 0;
            s_next = next;
        }
    } else if (threadIdx.x == 0) {                            // the final assignment ran in this step
        s.cur ^= 1;
        s_next = HMM_KM_SUM;
    }
    __syncthreads();
    const int next = s_next;
    if (next == HMM_KM_SUM) {
        const double inertia = sum_block(q.out, q.T, red);
        if (threadIdx.x == 0) {
            s.inertia = inertia;
            s.phase = HMM_KM_DONE;
            atomicAdd(done, 1);
        }
    } else if (threadIdx.x == 0) {
        s.phase = next;
    }
}

static int multi_grid(int64_t items, int cap)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>(items, cap));
}

void launch_hmm_multi_seed(const HmmKmProb* pr, HmmKmState* st, int n_prob, int max_rows, int kmeans, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_multi_seed, dim3(multi_grid((max_rows + 255) / 256, 256), n_prob), dim3(256), 0, s, pr, st, kmeans);
}

void launch_hmm_dist2_multi(const HmmKmProb* pr, int n_prob, int max_T, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_dist2_multi, dim3(multi_grid((max_T + 3) / 4, 1024), n_prob), dim3(256), 0, s, pr);
}

void launch_hmm_kmeans_multi_step(const HmmKmProb* pr, HmmKmState* st, int* done, int n_prob, int max_T, int max_items,
                                  int max_2d, hipStream_t s)
{
    hipLaunchKernelGGL(k_hmm_assign_multi, dim3(multi_grid((max_T + 3) / 4, 1024), n_prob), dim3(256), 0, s, pr, st);
    hipLaunchKernelGGL(k_hmm_colsum_multi, dim3(multi_grid(max_items, 4096), n_prob), dim3(kColThreads), 0, s, pr, st);
    hipLaunchKernelGGL(k_hmm_combine_multi, dim3(multi_grid((max_2d + 255) / 256, 1024), n_prob), dim3(256), 0, s, pr, st);
    hipLaunchKernelGGL(k_hmm_step_multi, dim3(n_prob), dim3(1024), 0, s, pr, st, done);
}

}  // namespace hicmi
