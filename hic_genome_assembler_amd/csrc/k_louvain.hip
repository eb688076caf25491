// k_louvain.hip - level 0 of the Louvain tail of Part 1 (scaffoldToChromosomes.py:239-349, modularity.py) on gfx950, fp64.
//
// The graph A (m x m, row-major, leading dimension m) is built once from the resident contact matrix.  Level 0 of every
// round runs in ONE launch, one workgroup per round: modularity._one_level(_Status(A), default_rng([seed, i])) restated
// bit for bit - the same node order, the same moves, the same fp64 operations in the same order, the same PCG64 draws
// (DESIGN.md section 9b).  Per-round state lives in LDS when it fits, else in a global slab of its own.
//
// The two sequential pieces of a node move:
//   * the uint32 draws of rng.permutation(present): lane t of the workgroup computes the LCG state t + 1 steps ahead
//     (a_t * s + c_t, jump constants computed once per launch) and its XSL-RR output, so a batch of 2 x 256 draws costs
//     one 128-bit multiply-add per lane; one lane then walks the batch applying random_interval's mask-and-reject.
//     Which community wins does not depend on the shuffle unless the best gain is tied, so the accepted swap indices
//     are only replayed (Fisher-Yates over the ascending community list) on a tie; the generator always advances by
//     exactly the draws the host consumes.
//   * np.bincount(node2com, weights=row): members are kept sorted by (community, node) in one array with a start
//     offset per community, so one lane per community sums its members' weights in ascending node order; a move
//     rotates the span between the old and the new slot by one.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "hicmi_internal.h"

namespace hicmi {

typedef unsigned __int128 u128;

static constexpr double kLvLn10 = 2.302585092994046;        // math.log(10), the divisor of modularity.log_transform
static constexpr double kLvMin = 0.0000001;                 // python-louvain __MIN
static constexpr int LV_T = 256;                            // threads of the level-0 workgroup
static constexpr int LV_W = LV_T / 64;
static constexpr int LV_CHAIN = 16;                         // member weights loaded ahead of a community's serial sum
static constexpr u128 kPcgMult = ((u128)0x2360ED051FC65DA4ull << 64) | (u128)0x4385DF649FCCF645ull;

// ---- graph build: A[i][j] = L[max(i, j)][min(i, j)], L = log10(sim + 1) (0 where sim == 0) of the tail rows
__device__ __forceinline__ double lv_similarity(double c, double sig, double rs)
{
    double d = (1.0 - (c / sig)) + 1.0;                       // the cell of k_sort.hip's similarity(), S2C:147-149
    return rs * (1.0 - (d - 1.0));
}

__global__ __launch_bounds__(256) void k_lv_graph(const double* __restrict__ C, int64_t ldc, const int32_t* __restrict__ rows,
                                                  const double* __restrict__ np_sum, const double* __restrict__ seq_sum, int m,
                                                  double* __restrict__ A)
{
    const int i = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (i >= m || j >= m) return;
    const int r = i > j ? i : j, q = i > j ? j : i;           // the later row's cell (add_edge overwrites, S2C:285-297)
    const int pa = rows[r];
    const double s = lv_similarity(C[(int64_t)pa * ldc + rows[q]], np_sum[pa], seq_sum[pa]);
    A[(int64_t)i * m + j] = s != 0.0 ? log(s + 1.0) / kLvLn10 : 0.0;
}

__global__ __launch_bounds__(256) void k_lv_diag(const double* __restrict__ A, int m, double* __restrict__ diag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) diag[i] = A[(int64_t)i * m + i];
}

// _Status.__init__: total_weight = (A.sum() + diag.sum()) / 2 and gdegrees = A.sum(axis=1) + diag, from NumPy's pairwise
// partial sums (chunk[] = the 8192-element chunks of the flattened A, accumulated left to right from 0.0)
__global__ __launch_bounds__(256) void k_lv_status(const double* __restrict__ rowsum, const double* __restrict__ diag,
                                                   const double* __restrict__ chunk, int n_chunks, const double* __restrict__ dsum,
                                                   int m, double* __restrict__ gdeg, double* __restrict__ total)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) gdeg[i] = rowsum[i] + diag[i];
    if (i == 0) {
        double acc = 0.0;
        for (int k = 0; k < n_chunks; k++) acc += chunk[k];
        total[0] = (acc + dsum[0]) / 2.0;
    }
}

// ---- PCG64 (numpy's XSL-RR 128/64)
__device__ __forceinline__ uint64_t pcg_output(u128 s)
{
    const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
    const unsigned rot = (unsigned)(hi >> 58);
    const uint64_t x = hi ^ lo;
    return (x >> rot) | (x << ((64u - rot) & 63u));
}

// s -> am * s + ap advances the LCG by `delta` steps (pcg_advance_lcg_128)
__device__ inline void pcg_jump(uint64_t delta, u128 inc, u128& am, u128& ap)
{
    u128 cm = kPcgMult, cp = inc;
    am = 1; ap = 0;
    while (delta) {
        if (delta & 1) { am *= cm; ap = ap * cm + cp; }
        cp = (cm + 1) * cp;
        cm *= cm;
        delta >>= 1;
    }
}

__device__ __forceinline__ uint32_t interval_mask(uint32_t v)
{
    v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
    return v;
}

struct LvShared {
    uint32_t buf[2 * LV_T + 1];
    uint64_t st_lo, st_hi, inc_lo, inc_hi;
    uint32_t has, uinteger;
    int done, consumed;                           // draw batch result
    int node, cn, best, ncom, modified, stop, shift_lo, shift_hi, shift_dir, q;
    double degc, rc, links;
    double red_max[LV_W];
    int red_cnt[LV_W], red_arg[LV_W], red_nan[LV_W];
    double maxv;
    int cnt, arg, nan;
};

__device__ __forceinline__ u128 lv_state(const LvShared& S) { return ((u128)S.st_hi << 64) | S.st_lo; }

// `top` calls of random_interval(i), i = top .. 1 (Generator.shuffle of top + 1 items): rec[i] = the accepted index.
// Every thread calls it (block-uniform `top`); the generator state in S advances exactly as numpy's does.
__device__ void lv_draws(LvShared& S, int top, int* rec, u128 jm, u128 jp)
{
    if (top <= 0) return;                                   // a permutation of 0 or 1 items draws nothing
    int i = top;                                            // (thread 0's copy is the live one)
    uint32_t mask = interval_mask((uint32_t)top);
    const int tid = threadIdx.x;
    for (;;) {
        const u128 s = lv_state(S);
        const int off = S.has ? 1 : 0;
        const u128 sn = jm * s + jp;                        // state tid + 1 steps ahead
        const uint64_t o = pcg_output(sn);
        S.buf[off + 2 * tid] = (uint32_t)o;                 // next_uint32: the low half first, the high half buffered
        S.buf[off + 2 * tid + 1] = (uint32_t)(o >> 32);
        if (tid == 0 && off) S.buf[0] = S.uinteger;
        __syncthreads();
        if (tid == 0) {
            const int n = off + 2 * LV_T;
            int c = 0;
            while (c < n && i > 0) {                        // 8 values read ahead of the serial mask-and-reject
                uint32_t w[8];
#pragma unroll
                for (int q = 0; q < 8; q++) w[q] = S.buf[min(c + q, n - 1)];
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    if (c < n && i > 0) {
                        const uint32_t v = w[q] & mask;
                        c++;
                        if (v <= (uint32_t)i) {
                            rec[i] = (int)v;
                            i--;
                            mask = interval_mask((uint32_t)i);
                        }
                    }
                }
            }
            S.consumed = c - off;                           // values of this batch's outputs taken (may be -1 or 0)
            S.done = i == 0;
            if (c > 0 && off) S.has = 0;                    // the buffered half was used
        }
        __syncthreads();
        const int used = S.consumed;
        const int q = used > 0 ? (used + 1) / 2 : 0;        // outputs generated by numpy
        if (q > 0 && tid == q - 1) {
            S.st_lo = (uint64_t)sn; S.st_hi = (uint64_t)(sn >> 64);
            S.has = used & 1;
            S.uinteger = (uint32_t)(o >> 32);
        }
        const int done = S.done;
        __syncthreads();
        if (done) return;
    }
}

// st.modularity(): communities in ascending id, res += internals / links - (degrees / (2 links))^2.  (The host squares
// with libm pow(); the device with x * x - see DESIGN.md: only this pass-termination value can differ, by an ulp.)
__device__ double lv_modularity(const int* sizes, const double* degrees, const double* internals, int m, double links)
{
    if (links <= 0.0) return 0.0;
    double res = 0.0;
    for (int c = 0; c < m; c++) {
        if (sizes[c] > 0) {
            const double a = degrees[c] / (2.0 * links);
            res += internals[c] / links - a * a;
        }
    }
    return res;
}

// One workgroup per round.  st: 6 uint64 per round (state lo, hi, inc lo, hi, has_uint32, uinteger); info: 4 int32 per
// round (passes, tie replays, near-threshold pass tests, 0).  Work arrays: LDS (lds = 1) or scratch + round * bytes.
__global__ __launch_bounds__(LV_T) void k_lv_level0(const double* __restrict__ A, int m, const double* __restrict__ gdeg,
                                                    const double* __restrict__ loops, const double* __restrict__ total,
                                                    const uint64_t* __restrict__ st_in, int32_t* __restrict__ n2c_out,
                                                    uint64_t* __restrict__ st_out, int32_t* __restrict__ info,
                                                    double* __restrict__ deg_out, double* __restrict__ int_out,
                                                    unsigned char* __restrict__ scratch, int lds)
{
    extern __shared__ __align__(16) unsigned char lv_dyn[];
    __shared__ LvShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = blockIdx.x;
    unsigned char* base = lds ? lv_dyn : scratch + (size_t)r * louvain_round_bytes(m);
    double* degrees = reinterpret_cast<double*>(base);
    double* internals = degrees + m;
    double* wto = internals + m;
    double* incr = wto + m;
    int* n2c = reinterpret_cast<int*>(incr + m);
    int* sizes = n2c + m;
    int* start = sizes + m;                     // first slot of community c in mem (communities in ascending id)
    int* mem = start + m;                       // nodes sorted by (community, node)
    int* pos = mem + m;                         // slot of node in mem
    int* perm = pos + m;                        // this pass's node order
    int* rec = perm + m;                        // accepted swap indices of the last draws
    int* tmp = rec + m;                         // tie-replay list / rotation buffer

    for (int c = tid; c < m; c += LV_T) {
        n2c[c] = c; sizes[c] = 1; start[c] = c; mem[c] = c; pos[c] = c;
        degrees[c] = gdeg[c]; internals[c] = loops[c];
    }
    if (tid == 0) {
        const uint64_t* si = st_in + 6 * r;
        S.st_lo = si[0]; S.st_hi = si[1]; S.inc_lo = si[2]; S.inc_hi = si[3];
        S.has = (uint32_t)si[4]; S.uinteger = (uint32_t)si[5];
        S.ncom = m; S.links = total[0];
    }
    __syncthreads();
    u128 jm, jp;
    pcg_jump((uint64_t)tid + 1, ((u128)S.inc_hi << 64) | S.inc_lo, jm, jp);
    const double links = S.links;
    double new_mod = 0.0;
    if (tid == 0) new_mod = lv_modularity(sizes, degrees, internals, m, links);
    int passes = 0, ties = 0, near = 0;
    int modified = 1;
    while (modified) {
        passes++;
        double cur_mod = new_mod;
        modified = 0;
        // rng.permutation(n): Fisher-Yates on arange(n) with the recorded indices
        lv_draws(S, m - 1, rec, jm, jp);
        if (tid == 0) {
            for (int k = 0; k < m; k++) perm[k] = k;
            for (int i = m - 1; i >= 1; i--) { const int j = rec[i]; const int t = perm[i]; perm[i] = perm[j]; perm[j] = t; }
        }
        __syncthreads();
        for (int idx = 0; idx < m; idx++) {
            if (tid == 0) {
                const int node = perm[idx], cn = n2c[node];
                S.node = node; S.cn = cn;
                if (--sizes[cn] == 0) S.ncom--;
                S.degc = gdeg[node] / (links * 2.0);
            }
            __syncthreads();
            const int node = S.node, cn = S.cn;
            const double* __restrict__ row = A + (int64_t)node * m;
            // w_to = np.bincount(node2com, weights=row) with row[node] = 0: ascending node order per community
            for (int c = tid; c < m; c += LV_T) {
                const int len = sizes[c] + (c == cn ? 1 : 0);
                if (len == 0) continue;
                // (adding row[node] = 0.0 as bincount does; the loads of 16 members are in flight before their adds)
                double acc = 0.0;
                int k = start[c];
                const int e = k + len;
                for (; k + LV_CHAIN <= e; k += LV_CHAIN) {
                    int j[LV_CHAIN];
                    double v[LV_CHAIN];
#pragma unroll
                    for (int q = 0; q < LV_CHAIN; q++) j[q] = mem[k + q];
#pragma unroll
                    for (int q = 0; q < LV_CHAIN; q++) v[q] = row[j[q]];
#pragma unroll
                    for (int q = 0; q < LV_CHAIN; q++) acc += j[q] != node ? v[q] : 0.0;
                }
                for (; k < e; k++) { const int j = mem[k]; acc += j != node ? row[j] : 0.0; }
                wto[c] = acc;
            }
            __syncthreads();
            if (tid == 0) {
                const double w_own = sizes[cn] > 0 ? wto[cn] : 0.0;
                S.rc = -w_own + (degrees[cn] - gdeg[node]) * S.degc;
                degrees[cn] -= gdeg[node];                  // __remove
                internals[cn] -= w_own + loops[node];
            }
            __syncthreads();
            // incr over the present communities: max, how many reach it, one that does, any NaN (np.argmax stops at
            // the first NaN, which then fails the `> 0` test)
            const double rc = S.rc, degc = S.degc;
            double bm = -INFINITY;
            int bc = 0, ba = -1, bn = 0;
            for (int c = tid; c < m; c += LV_T) {
                if (sizes[c] <= 0) continue;
                const double v = (rc + wto[c]) - degrees[c] * degc;
                incr[c] = v;
                if (v != v) bn = 1;
                else if (v > bm) { bm = v; bc = 1; ba = c; }
                else if (v == bm) bc++;
            }
            for (int o = 32; o >= 1; o >>= 1) {
                const double om = __shfl_xor(bm, o, 64);
                const int oc = __shfl_xor(bc, o, 64), oa = __shfl_xor(ba, o, 64), on = __shfl_xor(bn, o, 64);
                if (om > bm) { bm = om; bc = oc; ba = oa; }
                else if (om == bm) bc += oc;
                bn |= on;
            }
            if (lane == 0) { S.red_max[wave] = bm; S.red_cnt[wave] = bc; S.red_arg[wave] = ba; S.red_nan[wave] = bn; }
            __syncthreads();
            if (tid == 0) {
                double m0 = S.red_max[0];
                int c0 = S.red_cnt[0], a0 = S.red_arg[0], n0 = S.red_nan[0];
                for (int w = 1; w < LV_W; w++) {
                    if (S.red_max[w] > m0) { m0 = S.red_max[w]; c0 = S.red_cnt[w]; a0 = S.red_arg[w]; }
                    else if (S.red_max[w] == m0) c0 += S.red_cnt[w];
                    n0 |= S.red_nan[w];
                }
                S.maxv = m0; S.cnt = c0; S.arg = a0; S.nan = n0;
            }
            __syncthreads();
            const int P = S.ncom;
            __syncthreads();                                // (thread 0 changes ncom below, maybe without a draw barrier)
            lv_draws(S, P - 1, rec, jm, jp);                // rng.permutation(present)
            if (tid == 0) {
                int best = cn;
                if (!S.nan && P > 0 && S.maxv > 0.0) {
                    if (S.cnt == 1) {
                        best = S.arg;
                    } else {                                // tie: the first maximum in the shuffled order
                        int k = 0;
                        for (int c = 0; c < m; c++) if (sizes[c] > 0) tmp[k++] = c;
                        for (int i = P - 1; i >= 1; i--) { const int j = rec[i]; const int t = tmp[i]; tmp[i] = tmp[j]; tmp[j] = t; }
                        for (k = 0; k < P; k++) if (incr[tmp[k]] == S.maxv) { best = tmp[k]; break; }
                        ties++;
                    }
                }
                // __insert
                const double w_best = sizes[best] > 0 ? wto[best] : 0.0;
                n2c[node] = best;
                const int bsize = sizes[best];
                if (bsize == 0) S.ncom++;
                sizes[best] = bsize + 1;
                degrees[best] += gdeg[node];
                internals[best] += w_best + loops[node];
                S.best = best;
                if (best != cn) {
                    modified = 1;
                    // slot of node among best's members (sorted): binary search
                    int lo = start[best], hi = start[best] + bsize;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (mem[mid] < node) lo = mid + 1; else hi = mid; }
                    const int p_old = pos[node];
                    if (cn < best) { S.shift_lo = p_old; S.shift_hi = lo - 1; S.shift_dir = -1; }   // slots (p_old, q] move down
                    else { S.shift_lo = lo; S.shift_hi = p_old; S.shift_dir = 1; }                   // slots [q, p_old) move up
                }
            }
            __syncthreads();
            const int best = S.best;
            if (best != cn) {
                const int lo = S.shift_lo, hi = S.shift_hi, dir = S.shift_dir;
                for (int k = lo + tid; k <= hi; k += LV_T) tmp[k - lo] = mem[k];
                const int clo = dir < 0 ? cn + 1 : best + 1, chi = dir < 0 ? best : cn;
                for (int c = clo + tid; c <= chi; c += LV_T) start[c] += dir;
                __syncthreads();
                const int span = hi - lo + 1;
                for (int k = tid; k < span; k += LV_T) {
                    int dst, v;
                    if (dir < 0) { v = tmp[k]; dst = k == 0 ? hi : lo + k - 1; }     // tmp[0] is the node
                    else { v = tmp[k]; dst = k == span - 1 ? lo : lo + k + 1; }      // tmp[span - 1] is the node
                    mem[dst] = v;
                    pos[v] = dst;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            new_mod = lv_modularity(sizes, degrees, internals, m, links);
            const double gain = new_mod - cur_mod;
            if (fabs(gain - kLvMin) <= 1e-12) near++;
            S.stop = gain < kLvMin;
            S.modified = modified;
        }
        __syncthreads();
        modified = S.modified;
        if (S.stop) break;
        __syncthreads();
    }
    for (int c = tid; c < m; c += LV_T) {
        n2c_out[(size_t)r * m + c] = n2c[c];
        deg_out[(size_t)r * m + c] = degrees[c];
        int_out[(size_t)r * m + c] = internals[c];
    }
    if (tid == 0) {
        uint64_t* so = st_out + 6 * r;
        so[0] = S.st_lo; so[1] = S.st_hi; so[2] = S.inc_lo; so[3] = S.inc_hi; so[4] = S.has; so[5] = S.uinteger;
        int32_t* inf = info + 4 * r;
        inf[0] = passes; inf[1] = ties; inf[2] = near; inf[3] = 0;
    }
}

// ---- round aggregation (modularity._induced) and score (modularity.modularity), fixed orders of their own.
// members / moff: the nodes of every community in ascending node order (host-built CSR of the partition, k groups).
// rowagg[i][b] = sum over members j of b of A[i][j]
__global__ __launch_bounds__(256) void k_lv_rowagg(const double* __restrict__ A, int m, const int32_t* __restrict__ members,
                                                   const int32_t* __restrict__ moff, int k, double* __restrict__ rowagg)
{
    const int i = blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= k) return;
    const double* __restrict__ row = A + (int64_t)i * m;
    double acc = 0.0;
    for (int t = moff[b]; t < moff[b + 1]; t++) acc += row[members[t]];
    rowagg[(int64_t)i * k + b] = acc;
}

// B[a][b] = sum over members i of a of rowagg[i][b]; the diagonal becomes (B[a][a] + sum of the members' self loops) / 2
__global__ __launch_bounds__(256) void k_lv_induced(const double* __restrict__ A, int m, const double* __restrict__ rowagg,
                                                    const int32_t* __restrict__ members, const int32_t* __restrict__ moff, int k,
                                                    double* __restrict__ B)
{
    const int a = blockIdx.y;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= k) return;
    double acc = 0.0;
    for (int t = moff[a]; t < moff[a + 1]; t++) acc += rowagg[(int64_t)members[t] * k + b];
    if (a == b) {
        double loops = 0.0;
        for (int t = moff[a]; t < moff[a + 1]; t++) { const int i = members[t]; loops += A[(int64_t)i * m + i]; }
        acc = (acc + loops) / 2.0;
    }
    B[(int64_t)a * k + b] = acc;
}

// same[r][i] = sum over j with part_r[j] == part_r[i] of A[i][j] (a fixed-order block reduction)
__global__ __launch_bounds__(256) void k_lv_same(const double* __restrict__ A, int m, const int32_t* __restrict__ parts,
                                                 double* __restrict__ same)
{
    __shared__ double red[256];
    const int i = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int32_t* __restrict__ p = parts + (size_t)r * m;
    const int pi = p[i];
    const double* __restrict__ row = A + (int64_t)i * m;
    double acc = 0.0;
    for (int j = tid; j < m; j += 256) if (p[j] == pi) acc += row[j];
    red[tid] = acc;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) same[(size_t)r * m + i] = red[0];
}

// Q of round r: per community inc = (internal sum + self loops) / 2 and degree sum, in ascending node order, then
// res += inc / links - (deg / (2 links))^2 in ascending community id.  acc: 3 m doubles of scratch per round.
__global__ __launch_bounds__(64) void k_lv_score(const double* __restrict__ A, int m, const int32_t* __restrict__ parts,
                                                 const double* __restrict__ same, const double* __restrict__ gdeg,
                                                 const double* __restrict__ total, double* __restrict__ acc, double* __restrict__ q)
{
    const int r = blockIdx.x;
    if (threadIdx.x != 0) return;
    const int32_t* __restrict__ p = parts + (size_t)r * m;
    double* inc = acc + (size_t)r * 3 * m;
    double* deg = inc + m;
    double* present = deg + m;
    for (int c = 0; c < m; c++) { inc[c] = 0.0; deg[c] = 0.0; present[c] = 0.0; }
    for (int i = 0; i < m; i++) {
        const int c = p[i];
        inc[c] += same[(size_t)r * m + i] + A[(int64_t)i * m + i];
        deg[c] += gdeg[i];
        present[c] = 1.0;
    }
    const double links = total[0];
    double res = 0.0;
    for (int c = 0; c < m; c++) {
        if (present[c] == 0.0) continue;
        const double a = deg[c] / (2.0 * links);
        res += (inc[c] / 2.0) / links - a * a;
    }
    q[r] = res;
}

// ---- launchers
void launch_louvain_graph(const double* C, int64_t ldc, const int32_t* rows, const double* np_sum, const double* seq_sum, int m,
                          double* A, hipStream_t s)
{
    hipLaunchKernelGGL(k_lv_graph, dim3((m + 255) / 256, m), dim3(256), 0, s, C, ldc, rows, np_sum, seq_sum, m, A);
}

void launch_louvain_status(const double* A, int m, double* diag, double* rowsum, double* chunk, double* dsum, double* gdeg,
                           double* total, hipStream_t s)
{
    hipLaunchKernelGGL(k_lv_diag, dim3((m + 255) / 256), dim3(256), 0, s, A, m, diag);
    launch_pairwise_rows(A, m, m, m, rowsum, s);                         // A.sum(axis=1)
    const int64_t nn = (int64_t)m * m, full = nn / 8192, rem = nn % 8192;
    if (full > 0) launch_pairwise_rows(A, 8192, 8192, (int)full, chunk, s);   // A.sum(): 8192-element chunks
    if (rem > 0) launch_pairwise_rows(A + full * 8192, rem, (int)rem, 1, chunk + full, s);
    launch_pairwise_rows(diag, m, m, 1, dsum, s);                          // diag.sum()
    hipLaunchKernelGGL(k_lv_status, dim3((m + 255) / 256), dim3(256), 0, s, rowsum, diag, chunk, (int)(full + (rem > 0)), dsum,
                       m, gdeg, total);
}

int louvain_level0_lds_max()
{
    return 160 * 1024 - (int)sizeof(LvShared) - 1024;
}

void launch_louvain_level0(const double* A, int m, const double* gdeg, const double* loops, const double* total, int rounds,
                           const uint64_t* st_in, int32_t* n2c_out, uint64_t* st_out, int32_t* info, double* deg_out,
                           double* int_out, unsigned char* scratch, hipStream_t s)
{
    static std::atomic<int> have{0};
    const size_t bytes = louvain_round_bytes(m);
    const int lds = scratch == nullptr;
    if (lds) ensure_dynamic_lds(reinterpret_cast<const void*>(k_lv_level0), have, bytes);
    hipLaunchKernelGGL(k_lv_level0, dim3(rounds), dim3(LV_T), lds ? bytes : 0, s, A, m, gdeg, loops, total, st_in, n2c_out,
                       st_out, info, deg_out, int_out, scratch, lds);
}

void launch_louvain_induced(const double* A, int m, const int32_t* members, const int32_t* moff, int k, double* rowagg,
                            double* B, hipStream_t s)
{
    hipLaunchKernelGGL(k_lv_rowagg, dim3((k + 255) / 256, m), dim3(256), 0, s, A, m, members, moff, k, rowagg);
    hipLaunchKernelGGL(k_lv_induced, dim3((k + 255) / 256, k), dim3(256), 0, s, A, m, rowagg, members, moff, k, B);
}

void launch_louvain_score(const double* A, int m, const int32_t* parts, int rounds, const double* gdeg, const double* total,
                          double* same, double* acc, double* q, hipStream_t s)
{
    hipLaunchKernelGGL(k_lv_same, dim3(m, rounds), dim3(256), 0, s, A, m, parts, same);
    hipLaunchKernelGGL(k_lv_score, dim3(rounds), dim3(64), 0, s, A, m, parts, same, gdeg, total, acc, q);
}

}  // namespace hicmi
