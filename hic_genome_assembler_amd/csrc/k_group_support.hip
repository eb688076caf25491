// k_group_support.hip - group support of a Part 1 grouping (hicmi_group_sums).
//
// For every bin i and every chromosome group g the contact of i to the bins of g outside i's own scaffold is wanted,
//     binsum[i][g] = sum of M[j][i] over the rows j with grp[j] == g and scaf[j] != scaf[i],
// and per scaffold s the sum of binsum over its bins: one pass over the grouped rows of the n x n map (2 GB at 16,000
// bins, an HBM stream: the map does not fit the Infinity Cache).  The summation order is part of the definition: the
// members of g by ascending row index in chunks of GS_CHUNK, every chunk from 0.0 left to right, the chunk sums left to
// right, a scaffold's bins left to right in bin-list order.  The host sorts the rows by group and cuts the chunks.
//   k_gs_partial  one workgroup per (chunk, tile of 512 columns), one lane per pair of adjacent columns: it walks the
//                 chunk's rows in order - every row a coalesced stream of 16-byte loads, scaf[j] uniform per row - and
//                 writes one partial per (chunk, column).  No LDS, no atomics; every grouped row is read once.
//   k_gs_reduce   one workgroup per scaffold: binsum of its bins = the chunk partials of each group in chunk order, then
//                 scafsum = its bins in order, one lane per group.
//   k_gs_plain    HICMI_GROUP_SUPPORT_PLAIN=1, the A/B: one thread per (column, group) walks the same chunks in the same
//                 order with 8-byte loads and writes binsum itself (k_gs_reduce then only adds the scaffolds' bins).
// The 16-byte loads need an even leading dimension and a 16-byte aligned base (an odd n, or an adopted matrix at an odd
// offset, takes the 8-byte form of the same kernel).
#include "hicmi_internal.h"

namespace hicmi {

static constexpr int GS_TILE = 512;           // columns per workgroup of k_gs_partial: 256 lanes x 2

template <bool VEC>
__global__ __launch_bounds__(256) void k_gs_partial(const double* __restrict__ C, int64_t ld, int n,
                                                    const int32_t* __restrict__ rows, const GsChunk* __restrict__ chunks,
                                                    const int32_t* __restrict__ scaf, double* __restrict__ partial)
{
    const GsChunk ch = chunks[blockIdx.x];
    const int col = blockIdx.y * GS_TILE + 2 * threadIdx.x;
    if (col >= n) return;
    const bool two = col + 1 < n;                         // false in one lane at most: the last column of an odd n
    const int s0 = scaf[col], s1 = two ? scaf[col + 1] : -1;
    const int32_t* __restrict__ r = rows + ch.row0;
    const double* __restrict__ base = C + col;
    double a0 = 0.0, a1 = 0.0;
    if (two) {
#pragma unroll 8
        for (int k = 0; k < ch.cnt; k++) {
            const int j = r[k];                           // uniform: the row and its scaffold
            const int sj = scaf[j];
            const double* p = base + (int64_t)j * ld;
            double v0, v1;
            if (VEC) {
                const double2 v = *reinterpret_cast<const double2*>(p);
                v0 = v.x; v1 = v.y;
            } else {
                v0 = p[0]; v1 = p[1];
            }
            a0 += sj != s0 ? v0 : 0.0;                    // a scaffold's own bins never vote for it
            a1 += sj != s1 ? v1 : 0.0;
        }
    } else {
        for (int k = 0; k < ch.cnt; k++) {
            const int j = r[k];
            a0 += scaf[j] != s0 ? base[(int64_t)j * ld] : 0.0;
        }
    }
    double* __restrict__ out = partial + (int64_t)blockIdx.x * n + col;
    out[0] = a0;
    if (two) out[1] = a1;
}

__global__ __launch_bounds__(256) void k_gs_plain(const double* __restrict__ C, int64_t ld, int n, int G,
                                                  const int32_t* __restrict__ rows, const GsChunk* __restrict__ chunks,
                                                  const int32_t* __restrict__ group_chunk0, const int32_t* __restrict__ scaf,
                                                  double* __restrict__ binsum)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;       // columns fastest: a row is read coalesced
    if (t >= (int64_t)n * G) return;
    const int g = (int)(t / n), i = (int)(t - (int64_t)g * n);
    const int si = scaf[i];
    double total = 0.0;
    for (int c = group_chunk0[g]; c < group_chunk0[g + 1]; c++) {
        const GsChunk ch = chunks[c];
        double acc = 0.0;
        for (int k = 0; k < ch.cnt; k++) {
            const int j = rows[ch.row0 + k];
            const double v = C[(int64_t)j * ld + i];
            acc += scaf[j] != si ? v : 0.0;
        }
        total += acc;
    }
    binsum[(int64_t)i * G + g] = total;
}

// sbins: the bins sorted by scaffold (bin-list order inside a scaffold), soff[s] .. soff[s + 1] those of scaffold s
__global__ __launch_bounds__(256) void k_gs_reduce(const double* __restrict__ partial, int n, int G,
                                                   const int32_t* __restrict__ group_chunk0, const int32_t* __restrict__ sbins,
                                                   const int32_t* __restrict__ soff, double* binsum, double* __restrict__ scafsum,
                                                   int have_binsum)
{
    const int s = blockIdx.x;
    const int b0 = soff[s], L = soff[s + 1] - b0;
    if (!have_binsum) {
        const int64_t items = (int64_t)L * G;
        for (int64_t it = threadIdx.x; it < items; it += 256) {
            const int g = (int)(it / L), i = sbins[b0 + (int)(it - (int64_t)g * L)];     // bins fastest
            double acc = 0.0;
            for (int c = group_chunk0[g]; c < group_chunk0[g + 1]; c++) acc += partial[(int64_t)c * n + i];
            binsum[(int64_t)i * G + g] = acc;
        }
        __threadfence_block();
        __syncthreads();                                  // the scaffold's binsum rows were written by this workgroup
    }
    for (int g = threadIdx.x; g < G; g += 256) {
        double acc = 0.0;
        for (int b = 0; b < L; b++) acc += binsum[(int64_t)sbins[b0 + b] * G + g];
        scafsum[(int64_t)s * G + g] = acc;
    }
}

void launch_group_sums(const double* C, int64_t ld, int n, int G, int S, const int32_t* rows, const GsChunk* chunks,
                       int n_chunks, const int32_t* group_chunk0, const int32_t* scaf, const int32_t* sbins,
                       const int32_t* soff, double* partial, double* binsum, double* scafsum, bool plain, hipStream_t s)
{
    if (plain) {
        const int64_t threads = (int64_t)n * G;
        hipLaunchKernelGGL(k_gs_plain, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, C, ld, n, G, rows, chunks,
                           group_chunk0, scaf, binsum);
    } else if (n_chunks > 0) {
        const dim3 grid((unsigned)n_chunks, (unsigned)((n + GS_TILE - 1) / GS_TILE));
        const bool vec = (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0;
        if (vec) hipLaunchKernelGGL(k_gs_partial<true>, grid, dim3(256), 0, s, C, ld, n, rows, chunks, scaf, partial);
        else hipLaunchKernelGGL(k_gs_partial<false>, grid, dim3(256), 0, s, C, ld, n, rows, chunks, scaf, partial);
    }
    hipLaunchKernelGGL(k_gs_reduce, dim3((unsigned)S), dim3(256), 0, s, partial, n, G, group_chunk0, sbins, soff, binsum,
                       scafsum, plain ? 1 : 0);
}

}  // namespace hicmi
