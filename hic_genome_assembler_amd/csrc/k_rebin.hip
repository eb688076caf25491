// k_rebin.hip - a raw contact map summed to a coarser resolution (hicmi_rebin): the device side of a
// HiC-Pro `build_matrix` re-run at k times the bin size.
//
// group_start[0 .. m]: coarse bin I is the fine bins [group_start[I], group_start[I + 1]), at most REBIN_MAX_WIDTH of them.
//   R[I][J] = sum of C over rows of I x columns of J                    (I != J)
//   R[I][I] = sum of C[i][j] over i <= j, both in I                      (the block's upper triangle with its diagonal)
// One order for every kernel here, for I <= J:  p_j = the column sum of column j over the rows of I, top to bottom (in the
// diagonal block only the rows i <= j), then R[I][J] = p_j summed over the columns of J, left to right; R[J][I] is a copy
// of R[I][J], so R is exactly symmetric for any input.  No atomics: two runs give the same bits.
//   k_rebin         one 256-lane workgroup per coarse row I.  It walks the columns in chunks of REBIN_CHUNK: lane t owns the
//                   column pairs t and t + 256 of the chunk (16-byte loads), adds the rows of I into one accumulator per
//                   column and leaves the p_j in LDS; then one lane per coarse column that ENDS in the chunk adds its p_j
//                   (group_start drives it; a group that began in the chunk before finds its first columns still there,
//                   the LDS holds two chunks).  An odd n's last column is added alone, by the lane whose pair it opens.
//                   Only the chunks from group I's own columns on are read and only J >= I is written.
//   k_rebin_mirror  afterwards: the lower triangle from the upper one, 64 x 64 tiles through LDS, reads and writes both
//                   coalesced.
//   k_rebin_plain   HICMI_REBIN_PLAIN=1, the A/B: one thread per coarse cell looping over its block, the definition taken
//                   literally in the order above.
// The 16-byte form needs an even leading dimension and a 16-byte aligned base; otherwise the 8-byte form of the same
// kernel runs, with the same assignment of columns to lanes.
#include "hicmi_internal.h"

namespace hicmi {

static_assert(REBIN_CHUNK == 1024 && REBIN_MAX_WIDTH <= REBIN_CHUNK, "lane t owns the pairs t and t + 256 of a chunk");

// columns 2 p, 2 p + 1 of row r
template <bool VEC>
__device__ __forceinline__ double2 rebin_load_pair(const double* __restrict__ r, int p)
{
    if (VEC) return *reinterpret_cast<const double2*>(r + 2 * p);
    return make_double2(r[2 * p], r[2 * p + 1]);
}

// B consecutive rows from r on, added into the column accumulators of the lane's two pairs
template <bool VEC, int B>
__device__ __forceinline__ void rebin_add_rows(const double* __restrict__ r, int64_t ld, int p0, int p1, bool on0, bool on1,
                                               double& a0, double& a1, double& b0, double& b1)
{
    double2 va[B], vb[B];
#pragma unroll
    for (int u = 0; u < B; u++) {
        va[u] = on0 ? rebin_load_pair<VEC>(r + (int64_t)u * ld, p0) : make_double2(0.0, 0.0);
        vb[u] = on1 ? rebin_load_pair<VEC>(r + (int64_t)u * ld, p1) : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < B; u++) { a0 += va[u].x; a1 += va[u].y; b0 += vb[u].x; b1 += vb[u].y; }
}

// chunk_first[c]: the first coarse column whose last fine column lies in chunk c or later (chunk_first[n_chunks] = m)
template <bool VEC>
__global__ __launch_bounds__(256) void k_rebin(const double* __restrict__ C, int64_t ld, int n,
                                               const int32_t* __restrict__ group_start,
                                               const int32_t* __restrict__ chunk_first, int m, double* __restrict__ R)
{
    __shared__ __attribute__((aligned(16))) double s_col[2 * REBIN_CHUNK];
    const int I = blockIdx.x, t = threadIdx.x;
    const int gs = group_start[I], ge = group_start[I + 1];
    const int pairs = n >> 1;
    const int n_chunks = (n + REBIN_CHUNK - 1) / REBIN_CHUNK;
    const double* __restrict__ rows = C + (int64_t)gs * ld;
    for (int c = gs / REBIN_CHUNK; c < n_chunks; c++) {
        const int p0 = c * (REBIN_CHUNK / 2) + t, p1 = p0 + 256;
        const bool on0 = p0 < pairs, on1 = p1 < pairs;
        double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
        if (c * REBIN_CHUNK < ge && (c + 1) * REBIN_CHUNK > gs) {
            // the chunk holds columns of the diagonal block: column j takes the rows i <= j of its own group
            for (int i = gs; i < ge; i++) {
                const double* __restrict__ r = rows + (int64_t)(i - gs) * ld;
                if (on0) {
                    const double2 v = rebin_load_pair<VEC>(r, p0);
                    const int j = 2 * p0;
                    if (j < gs || j >= i) a0 += v.x;
                    if (j + 1 < gs || j + 1 >= i) a1 += v.y;
                }
                if (on1) {
                    const double2 v = rebin_load_pair<VEC>(r, p1);
                    const int j = 2 * p1;
                    if (j < gs || j >= i) b0 += v.x;
                    if (j + 1 < gs || j + 1 >= i) b1 += v.y;
                }
            }
        } else {
            // B rows of both pairs fetched ahead of their adds; each column's adds stay top to bottom
            int i = 0;
            const int w = ge - gs;
            for (; i + 4 <= w; i += 4) rebin_add_rows<VEC, 4>(rows + (int64_t)i * ld, ld, p0, p1, on0, on1, a0, a1, b0, b1);
            if (i + 2 <= w) { rebin_add_rows<VEC, 2>(rows + (int64_t)i * ld, ld, p0, p1, on0, on1, a0, a1, b0, b1); i += 2; }
            if (i < w) rebin_add_rows<VEC, 1>(rows + (int64_t)i * ld, ld, p0, p1, on0, on1, a0, a1, b0, b1);
        }
        // an odd n's last column, alone: the lane whose pair it opens adds it (it is at or right of every row's diagonal)
        if ((n & 1) && (p0 == pairs || p1 == pairs)) {
            double last = 0.0;
            for (int i = gs; i < ge; i++) last += rows[(int64_t)(i - gs) * ld + (n - 1)];
            if (p0 == pairs) a0 = last; else b0 = last;
        }
        double* __restrict__ half = s_col + (c & 1) * REBIN_CHUNK;
        *reinterpret_cast<double2*>(half + 2 * t) = make_double2(a0, a1);
        *reinterpret_cast<double2*>(half + 512 + 2 * t) = make_double2(b0, b1);
        __syncthreads();
        // the coarse columns that end in this chunk
        const int j_lo = chunk_first[c], j_hi = chunk_first[c + 1];
        for (int J = j_lo + t; J < j_hi; J += 256) {
            if (J < I) continue;
            const int s = group_start[J], e = group_start[J + 1];
            double acc = s_col[s & (2 * REBIN_CHUNK - 1)];
            for (int j = s + 1; j < e; j++) acc += s_col[j & (2 * REBIN_CHUNK - 1)];
            R[(int64_t)I * m + J] = acc;
        }
        __syncthreads();                                      // the next chunk overwrites the other half, read above
    }
}

__global__ __launch_bounds__(256) void k_rebin_mirror(double* __restrict__ R, int m)
{
    __shared__ double tile[64][65];
    const int bi = blockIdx.y, bj = blockIdx.x;               // the upper tile (bi, bj) goes to the lower tile (bj, bi)
    if (bj < bi) return;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int r = bi * 64 + i, c = bj * 64 + tx;
        tile[i][tx] = (r < m && c < m && r < c) ? R[(int64_t)r * m + c] : 0.0;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int r = bj * 64 + i, c = bi * 64 + tx;
        if (r < m && c < r) R[(int64_t)r * m + c] = tile[tx][i];
    }
}

__global__ __launch_bounds__(256) void k_rebin_plain(const double* __restrict__ C, int64_t ld,
                                                     const int32_t* __restrict__ group_start, int m, double* __restrict__ R)
{
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= (int64_t)m * m) return;
    const int a = (int)(cell / m), b = (int)(cell % m);
    const int I = a < b ? a : b, J = a < b ? b : a;
    const int is = group_start[I], ie = group_start[I + 1], js = group_start[J], je = group_start[J + 1];
    double acc = 0.0;
    for (int j = js; j < je; j++) {
        const int i_end = I == J ? j + 1 : ie;               // the diagonal block: the rows i <= j
        double p = 0.0;
        for (int i = is; i < i_end; i++) p += C[(int64_t)i * ld + j];
        acc = j == js ? p : acc + p;
    }
    R[cell] = acc;
}

static bool rebin_vec_ok(const double* C, int64_t ld) { return (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0; }

void launch_rebin(const double* C, int64_t ld, int n, const int32_t* group_start, const int32_t* chunk_first, int m,
                  double* R, bool plain, hipStream_t s)
{
    if (plain) {
        const int64_t cells = (int64_t)m * m;
        hipLaunchKernelGGL(k_rebin_plain, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, C, ld, group_start, m, R);
        return;
    }
    if (rebin_vec_ok(C, ld))
        hipLaunchKernelGGL(k_rebin<true>, dim3((unsigned)m), dim3(256), 0, s, C, ld, n, group_start, chunk_first, m, R);
    else
        hipLaunchKernelGGL(k_rebin<false>, dim3((unsigned)m), dim3(256), 0, s, C, ld, n, group_start, chunk_first, m, R);
    const unsigned tiles = (unsigned)((m + 63) / 64);
    hipLaunchKernelGGL(k_rebin_mirror, dim3(tiles, tiles), dim3(256), 0, s, R, m);
}

}  // namespace hicmi
