// k_ice.hip - ICE balancing of a raw contact map (hicmi_ice_mask_rows, hicmi_ice_balance): the device side
// of HiC-Pro's `ice` step.
//
// The iteration only ever needs the row sums s of the running matrix X, and X = C_ij / (bias_i bias_j) throughout, so
// with u = 1 / bias the row sums are s_i = u_i * sum_j C_ij u_j: one read-only pass over the raw map per iteration.
//   k_ice_rowdot  y_i = sum_j C_ij u_j, one 256-lane workgroup per row.  Lane t owns the column pairs t, t + 256, ...
//                 (16-byte loads of the row and of u), adds the products of its even columns into one accumulator and of
//                 its odd columns into another, left to right; then even + odd, the xor tree inside a wave, and
//                 (w0 + w1) + (w2 + w3) over the waves.  An odd n's last column is added by lane 0 after its pairs.  The
//                 order is a function of n alone - no atomics - so two runs give the same bits.
//   k_ice_vec_b   the vector half-step after a row pass: s = u * y, sum X = sum s, c, bias *= sqrt(c), sum |bias_prev -
//                 bias|, s /= c; one 1024-lane workgroup, every sum in lane-strided order + a fixed tree.  It leaves one
//                 (delta, c) record per iteration for the host.
//   k_ice_vec_a   the half-step before a row pass: mean of the non-zero s, d, bias *= d, u = 1 / bias.
//   k_ice_apply   once at the end: X_ij = C_ij * (u_i * u_j), in place (u_i * u_j commutes: X is exactly symmetric).
//   k_ice_scale   HICMI_ICE_INPLACE=1, the A/B: the definition taken literally, X_ij /= d_i d_j and X /= c in place each
//                 iteration; its row sums come from k_ice_rowdot with u = 1.
//   k_ice_mask    zero the masked rows and columns.
// The 16-byte forms need an even leading dimension and a 16-byte aligned base; otherwise the 8-byte form of the same
// kernel runs, with the same assignment of columns to lanes.
#include "hicmi_internal.h"

namespace hicmi {

static constexpr int ICE_VEC_LANES = 1024;

// all 1024 lanes get the sum: xor tree inside a wave, then the 16 wave sums left to right
__device__ __forceinline__ double ice_block_sum(double v, double* s_w)
{
    v = wave_sum_s(v);
    __syncthreads();                                      // s_w may still be read from the previous sum
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double acc = s_w[0];
#pragma unroll
    for (int w = 1; w < ICE_VEC_LANES / 64; w++) acc += s_w[w];
    return acc;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_ice_rowdot(const double* __restrict__ C, int64_t ld, int n,
                                                    const double* __restrict__ u, double* __restrict__ y)
{
    __shared__ double s_w[4];
    const int row = blockIdx.x;
    const double* __restrict__ r = C + (int64_t)row * ld;
    const int pairs = n >> 1;
    double a0 = 0.0, a1 = 0.0;
#pragma unroll 8
    for (int p = threadIdx.x; p < pairs; p += 256) {
        double c0, c1, u0, u1;
        if (VEC) {
            const double2 cv = *reinterpret_cast<const double2*>(r + 2 * p);
            c0 = cv.x; c1 = cv.y;
        } else {
            c0 = r[2 * p]; c1 = r[2 * p + 1];
        }
        const double2 uv = *reinterpret_cast<const double2*>(u + 2 * p);     // u is the library's own, aligned buffer
        u0 = uv.x; u1 = uv.y;
        a0 += c0 * u0;
        a1 += c1 * u1;
    }
    if ((n & 1) && threadIdx.x == 0) a0 += r[n - 1] * u[n - 1];
    const double sum = block_sum_256(a0 + a1, s_w);
    if (threadIdx.x == 0) y[row] = sum;
}

// st[0] = mean0, st[1] = the last c.  first: the pass over the raw map before iteration 0 (sets mean0 and s only).
__global__ __launch_bounds__(ICE_VEC_LANES) void k_ice_vec_b(int n, const double* __restrict__ y, double* __restrict__ u,
                                                             double* __restrict__ bias, double* __restrict__ prev,
                                                             double* __restrict__ s, double* __restrict__ st,
                                                             double* __restrict__ rec, int it, int first)
{
    __shared__ double s_w[ICE_VEC_LANES / 64];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int i = tid; i < n; i += ICE_VEC_LANES) {
        const double v = u ? u[i] * y[i] : y[i];
        s[i] = v;
        acc += v;
    }
    const double tot = ice_block_sum(acc, s_w);
    const double nn = (double)n * (double)n;
    if (first) {
        if (tid == 0) { st[0] = tot / nn; st[1] = 1.0; }
        return;
    }
    const double c = (tot / nn) / st[0];
    const double sc = sqrt(c);
    double dl = 0.0;
    for (int i = tid; i < n; i += ICE_VEC_LANES) {
        const double b = bias[i] * sc;
        dl += fabs(prev[i] - b);
        bias[i] = b;
        prev[i] = b;
        if (u) {
            s[i] = s[i] / c;                              // the row sums of X / c (the in-place path sums them again)
            u[i] = 1.0 / b;                               // X = C_ij u_i u_j holds after every half-step (k_ice_apply)
        }
    }
    const double delta = ice_block_sum(dl, s_w);
    if (tid == 0) { rec[2 * it] = delta; rec[2 * it + 1] = c; st[1] = c; }
}

// s: the row sums of X.  u == nullptr: the in-place path (d is what k_ice_scale divides by).
__global__ __launch_bounds__(ICE_VEC_LANES) void k_ice_vec_a(int n, const double* __restrict__ s, double* __restrict__ bias,
                                                             double* __restrict__ u, double* __restrict__ d)
{
    __shared__ double s_w[ICE_VEC_LANES / 64];
    const int tid = threadIdx.x;
    double acc = 0.0, cnt = 0.0;
    for (int i = tid; i < n; i += ICE_VEC_LANES) {
        const double v = s[i];
        if (v != 0.0) { acc += v; cnt += 1.0; }
    }
    const double sum = ice_block_sum(acc, s_w);
    const double k = ice_block_sum(cnt, s_w);             // a count below 2^53: exact
    const double mean = k > 0.0 ? sum / k : 1.0;
    for (int i = tid; i < n; i += ICE_VEC_LANES) {
        const double v = s[i];
        const double di = v != 0.0 ? v / mean : 1.0;
        const double b = bias[i] * di;
        bias[i] = b;
        d[i] = di;
        if (u) u[i] = 1.0 / b;
    }
}

// row blockIdx.x of X, every element x at column j replaced by f(j, x); lane t owns the column pairs t, t + 256, ...
template <bool VEC, class F>
__device__ __forceinline__ void ice_row_map(double* __restrict__ X, int64_t ld, int n, F f)
{
    double* __restrict__ r = X + (int64_t)blockIdx.x * ld;
    const int pairs = n >> 1;
#pragma unroll 4
    for (int p = threadIdx.x; p < pairs; p += 256) {
        if (VEC) {
            double2 v = *reinterpret_cast<double2*>(r + 2 * p);
            v.x = f(2 * p, v.x); v.y = f(2 * p + 1, v.y);
            *reinterpret_cast<double2*>(r + 2 * p) = v;
        } else {
            r[2 * p] = f(2 * p, r[2 * p]);
            r[2 * p + 1] = f(2 * p + 1, r[2 * p + 1]);
        }
    }
    if ((n & 1) && threadIdx.x == 0) r[n - 1] = f(n - 1, r[n - 1]);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_ice_apply(double* __restrict__ X, int64_t ld, int n, const double* __restrict__ u)
{
    const double ui = u[blockIdx.x];
    ice_row_map<VEC>(X, ld, n, [=](int j, double x) { return x * (ui * u[j]); });
}

// by_c == 0: X_ij /= d_i d_j; by_c != 0: X /= c, c = st[1]
template <bool VEC>
__global__ __launch_bounds__(256) void k_ice_scale(double* __restrict__ X, int64_t ld, int n, const double* __restrict__ d,
                                                   const double* __restrict__ st, int by_c)
{
    if (by_c) {
        const double c = st[1];
        ice_row_map<VEC>(X, ld, n, [=](int, double x) { return x / c; });
    } else {
        const double di = d[blockIdx.x];
        ice_row_map<VEC>(X, ld, n, [=](int j, double x) { return x / (di * d[j]); });
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_ice_mask(double* __restrict__ X, int64_t ld, int n, const uint8_t* __restrict__ mask)
{
    const bool mi = mask[blockIdx.x] != 0;
    ice_row_map<VEC>(X, ld, n, [=](int j, double x) { return (mi || mask[j]) ? 0.0 : x; });
}

__global__ __launch_bounds__(256) void k_ice_fill(double* __restrict__ v, int n, double value)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = value;
}

static bool ice_vec_ok(const double* C, int64_t ld) { return (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0; }

void launch_ice_fill(double* v, int n, double value, hipStream_t s)
{
    hipLaunchKernelGGL(k_ice_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, v, n, value);
}

void launch_ice_rowdot(const double* C, int64_t ld, int n, const double* u, double* y, hipStream_t s)
{
    if (ice_vec_ok(C, ld)) hipLaunchKernelGGL(k_ice_rowdot<true>, dim3((unsigned)n), dim3(256), 0, s, C, ld, n, u, y);
    else hipLaunchKernelGGL(k_ice_rowdot<false>, dim3((unsigned)n), dim3(256), 0, s, C, ld, n, u, y);
}

void launch_ice_vec_b(int n, const double* y, double* u, double* bias, double* prev, double* sums, double* st,
                      double* rec, int it, int first, hipStream_t s)
{
    hipLaunchKernelGGL(k_ice_vec_b, dim3(1), dim3(ICE_VEC_LANES), 0, s, n, y, u, bias, prev, sums, st, rec, it, first);
}

void launch_ice_vec_a(int n, const double* sums, double* bias, double* u, double* d, hipStream_t s)
{
    hipLaunchKernelGGL(k_ice_vec_a, dim3(1), dim3(ICE_VEC_LANES), 0, s, n, sums, bias, u, d);
}

void launch_ice_apply(double* X, int64_t ld, int n, const double* u, hipStream_t s)
{
    if (ice_vec_ok(X, ld)) hipLaunchKernelGGL(k_ice_apply<true>, dim3((unsigned)n), dim3(256), 0, s, X, ld, n, u);
    else hipLaunchKernelGGL(k_ice_apply<false>, dim3((unsigned)n), dim3(256), 0, s, X, ld, n, u);
}

void launch_ice_scale(double* X, int64_t ld, int n, const double* d, const double* st, int by_c, hipStream_t s)
{
    if (ice_vec_ok(X, ld)) hipLaunchKernelGGL(k_ice_scale<true>, dim3((unsigned)n), dim3(256), 0, s, X, ld, n, d, st, by_c);
    else hipLaunchKernelGGL(k_ice_scale<false>, dim3((unsigned)n), dim3(256), 0, s, X, ld, n, d, st, by_c);
}

void launch_ice_mask(double* X, int64_t ld, int n, const uint8_t* mask, hipStream_t s)
{
    if (ice_vec_ok(X, ld)) hipLaunchKernelGGL(k_ice_mask<true>, dim3((unsigned)n), dim3(256), 0, s, X, ld, n, mask);
    else hipLaunchKernelGGL(k_ice_mask<false>, dim3((unsigned)n), dim3(256), 0, s, X, ld, n, mask);
}

}  // namespace hicmi
