// hicmi_internal.h - shared declarations between the kernel translation units and api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <functional>

#include "liftmap.h"
#include "span.h"
#include "ends.h"
#include "anchor.h"
#include "pairs.h"
#include "seats.h"
#include "links.h"
#include "split.h"

namespace hicmi {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) only when a launch needs more than any earlier one
// (the call costs as much as a launch, and the search paths launch tens of thousands of kernels)
inline void ensure_dynamic_lds(const void* func, std::atomic<int>& have, size_t bytes)
{
    if ((int)bytes > have.load(std::memory_order_relaxed)) {
        (void)hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        have.store((int)bytes, std::memory_order_relaxed);
    }
}

// ---- strictly left-to-right fp64 chains over LDS (the reference's Python sum() / running sums cannot be
// re-associated).  One lane runs them; the next 8 operands are fetched while the current 8 are added, so
// the chain waits on the adder only.
static constexpr int SERIAL_BATCH = 16;                 // operands in flight: 16 dependent fp64 adds cover an LDS round trip

__device__ __forceinline__ double serial_sum_lds(const double* t, int from, int to, double acc)
{
    constexpr int B = SERIAL_BATCH;
    int i = from;
    if (i + B <= to) {
        double a[B];
#pragma unroll
        for (int q = 0; q < B; q++) a[q] = t[i + q];
        while (i + 2 * B <= to) {
            double b[B];
#pragma unroll
            for (int q = 0; q < B; q++) b[q] = t[i + B + q];
#pragma unroll
            for (int q = 0; q < B; q++) acc += a[q];
#pragma unroll
            for (int q = 0; q < B; q++) a[q] = b[q];
            i += B;
        }
#pragma unroll
        for (int q = 0; q < B; q++) acc += a[q];
        i += B;
    }
    for (; i < to; i++) acc += t[i];
    return acc;
}

// t[i] <- acc + t[from] + ... + t[i] for i in [from, to), left to right
__device__ __forceinline__ double serial_prefix_lds(double* t, int from, int to, double acc)
{
    constexpr int B = SERIAL_BATCH;
    int i = from;
    if (i + B <= to) {
        double a[B];
#pragma unroll
        for (int q = 0; q < B; q++) a[q] = t[i + q];
        while (i + 2 * B <= to) {
            double b[B];
#pragma unroll
            for (int q = 0; q < B; q++) b[q] = t[i + B + q];
#pragma unroll
            for (int q = 0; q < B; q++) { acc += a[q]; t[i + q] = acc; }
#pragma unroll
            for (int q = 0; q < B; q++) a[q] = b[q];
            i += B;
        }
#pragma unroll
        for (int q = 0; q < B; q++) { acc += a[q]; t[i + q] = acc; }
        i += B;
    }
    for (; i < to; i++) { acc += t[i]; t[i] = acc; }
    return acc;
}

// ---- NumPy's pairwise summation tree (add.reduce of one contiguous or strided run of <= 8192 elements) -----------
// An 8192-element chunk splits into 64 leaves, but a shorter one can split into 65: the left half is rounded down to a
// multiple of 8, so the right halves of 7,689 ... 8,191-element runs reach 129+ elements one level earlier
// (tests/test_host_cpu.py walks the recursion for every length up to 8192).
static constexpr int MAX_LEAVES = 65;

// Leaves of NumPy's pairwise recursion over [off, off+len), in order, with their depth in the
// recursion tree.  The explicit stack lives in LDS (st_off/st_len/st_dep: 16 entries each): private
// arrays indexed at run time would be spilled to scratch memory, a global-memory round trip per access.
__device__ __forceinline__ int enumerate_leaves(int off, int len, int* leaf_off, int* leaf_len, int* leaf_dep,
                                                int* st_off, int* st_len, int* st_dep)
{
    int sp = 1, n = 0;
    st_off[0] = off; st_len[0] = len; st_dep[0] = 0;
    while (sp > 0) {
        sp--;
        const int o = st_off[sp], l = st_len[sp], d = st_dep[sp];
        if (l <= 128) { leaf_off[n] = o; leaf_len[n] = l; leaf_dep[n] = d; n++; continue; }
        int n2 = l / 2;
        n2 -= n2 % 8;
        st_off[sp] = o + n2; st_len[sp] = l - n2; st_dep[sp] = d + 1; sp++;      // right half (processed second)
        st_off[sp] = o; st_len[sp] = n2; st_dep[sp] = d + 1; sp++;                // left half
    }
    return n;
}

// left + right at every split of the same tree: leaves arrive in order; whenever the two newest partial
// results sit at the same depth they are the two halves of one node (left first) and are replaced by
// their sum one level up.  val/dep: LDS stacks of 16 entries.
__device__ __forceinline__ double combine_leaves(int n_leaves, const double* leaf_sum, const int* leaf_dep, double* val,
                                                 int* dep)
{
    int sp = 0;
    for (int l = 0; l < n_leaves; l++) {
        double v = leaf_sum[l];
        int d = leaf_dep[l];
        while (sp > 0 && dep[sp - 1] == d) { v = val[sp - 1] + v; d--; sp--; }
        val[sp] = v; dep[sp] = d; sp++;
    }
    return val[0];
}

// ---- launchers (defined next to their kernels) --------------------------------------------------
// k_part1.hip
void launch_row_sums(const double* C, int64_t ldc, int n, double* np_sum, double* seq_sum, int row_first, int row_stride,
                     hipStream_t s);
void launch_pairwise_rows(const double* C, int64_t ldc, int len, int rows, double* out, hipStream_t s);
void launch_compact(const double* src, int64_t ld_src, const int32_t* keep, int n_keep, double* dst, int64_t ld_dst,
                    hipStream_t s);
void launch_widen_f32(const float* src, double* dst, int64_t cells, hipStream_t s);   // src = (float*)dst + cells
void launch_build_w(const double* C, int64_t ldc, const double* np_sum, int n, double* W, int64_t ldw, hipStream_t s);
// k_nnchain.hip
size_t nnchain_workspace_bytes(int n);
// Every HICMI_NNCHAIN_* switch, read once per hicmi_upgma call (README.md lists them)
struct NNChainOptions {
    bool profile = false;                     // _PROFILE: phase time stamps
    int dcap = 256;                           // _DCAP: merges per epoch of the 1024-lane kernels (clamped to 1 .. 1024)
    bool dcap_forced = false;                 //   ... and of the one-wave kernel's epochs too
    bool compact = true;                      // _NO_COMPACT turns compaction off
    bool wgs_set = false; int wgs = 0;        // _WGS: the 1024-lane kernels at this width (1, 2, 4, 8, 16) for every epoch
    bool plain = false;                       // _PLAIN: the cache-less k_nn_epoch
    bool gsize = false;                       // _GSIZE: k_nn_epoch_mwc's sizes-in-global-memory form at every width
    bool w1 = true;                           // _W1=0: not the one-wave kernel
    int w1_s = 0;                             // _W1_S: its number of slices (0: planned)
    int w1_cols = 0;                          // _W1_COLS: the columns per slice its plan aims at (at least 64)
    int w1_maxs = 0;                          // _W1_MAXS: its largest number of slices
    int xcc = -1;                             // _XCD: the XCD its parties claim (off: -1; 8: one that does not exist); unset: probed
    int test_late = 0, test_diverge = 0, test_rollcall = 0;     // _TEST_LATE, _TEST_DIVERGE, _TEST_ROLLCALL: test hooks
};
NNChainOptions nnchain_options(int probed_xcc);
int nnchain_probe_xcc(hipStream_t s);       // the lowest XCC id the device's workgroups report (once per device; waits on s)
int launch_nnchain(double* W, double* W2, int64_t ldw, int n, int* chain, double* zraw, void* workspace, const NNChainOptions& o,
                   int fallback, hipStream_t s, const std::function<void()>& after_first_rowmin = nullptr);
                                              // returns the number of epoch launches; fallback: 0, 1 (spread out), 2 (one workgroup);
                                              // after_first_rowmin: called once, when the first epoch's cache pass is queued
void launch_selftest_division(unsigned long long seed, int blocks, int iters, unsigned long long* d_mismatches, hipStream_t s);
const int* nnchain_state_ptr(void* workspace);                    // 16 ints: [0] merges done ... [5] stop code (0 = none,
                                                                  // 1 = guard / NaN, 2 = a peer workgroup answered late, 3 = replicas disagree)
const unsigned long long* nnchain_prof_ptr(void* workspace);      // 8 counters, contiguous after the state: [0..4] phase totals
                                                                  // (100 MHz ticks), [5] columns visited by scans, [6] scans, [7] cache hits
void launch_cut_count(const uint16_t* rank, int64_t ldr, int row0, int nrows, int lo, int mode, int cparam,
                      int32_t* x_out, int row_step, hipStream_t s);
void launch_hyper_flags(const int32_t* x, int nrows, int mode, int L_fixed, int64_t M, double psig, uint8_t* sig,
                        int own_first, int own_step, hipStream_t s);

// k_part1_scan.hip: the cut-scan loops with their control flow on the device, for up to SCAN_MAX_SETS parameter sets in
// lock step.  One record per set in device memory carries the arguments of its next scan and its loop state; the host
// reads the records back once per batch of scans.
struct ScanState {
    int done;              // the loop has ended: later launches return at once
    int mode;              // 0 first pass (S2C:413-551), 1 filter (S2C:553-727)
    int start, cut, n_rows, recount;
    long long M;
    double psig;           // the set's p-value threshold
    int min_size, stop_ind, loop_count, n_cuts, n_log, scans;          // first pass
    int MD, n_alt, alt_off, f_i, f_keep_from, f_noise, f_round, f_max_rounds, f_warned;   // filter
    int pad;
    unsigned long long bytes;                                           // rank bytes the scans' queries cover
};
// Records st[0..n_sets), per-set lists at k * n (mlog at k * 2n, seg at k * 3n).  One set counts through k_cut_rows (psig
// by value: st[0].psig); several through k_cut_rows_multi, where `share` lets sets that recount at the same arguments
// share the count.
static constexpr int SCAN_MAX_SETS = 64;
void launch_first_pass_multi_pairs(const uint16_t* rank, int64_t ldr, int n, int n_sets, ScanState* st, int32_t* x, uint8_t* sig,
                                   double psig0, int share, int32_t* cuts, int32_t* mlog, int log_cap, int pairs, hipStream_t s);
void launch_filter_multi_pairs(const uint16_t* rank, int64_t ldr, int n, int max_rows, int n_sets, ScanState* st, int32_t* x,
                               uint8_t* sig, double psig0, int share, int32_t* alt, uint8_t* filt, uint8_t* prev,
                               int32_t* seg, int32_t* seg_x, int pairs, hipStream_t s);

// The value lane ^ M holds, M a power of two below 64, without the LDS crossbar (ds_bpermute, which __shfl_xor compiles
// to, issues at a fraction of the VALU rate and was what the bitonic networks' in-wave stages waited for): DPP quad
// permutes and row mirrors inside a row of 16 lanes, gfx950's v_permlane16_swap / v_permlane32_swap across rows.
#if defined(__HIPCC__)
template <int M>
__device__ __forceinline__ uint32_t xor_lane(uint32_t v, int lane)
{
    if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xf, 0xf, true);       // quad_perm [1,0,3,2]
    else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xf, 0xf, true);  // quad_perm [2,3,0,1]
    else if constexpr (M == 4) {
        const int t = __builtin_amdgcn_mov_dpp((int)v, 0x141, 0xf, 0xf, true);                            // row_half_mirror: ^ 7
        return (uint32_t)__builtin_amdgcn_mov_dpp(t, 0x1B, 0xf, 0xf, true);                               // quad_perm [3,2,1,0]: ^ 3
    } else if constexpr (M == 8) {
        const int t = __builtin_amdgcn_mov_dpp((int)v, 0x140, 0xf, 0xf, true);                            // row_mirror: ^ 15
        return (uint32_t)__builtin_amdgcn_mov_dpp(t, 0x141, 0xf, 0xf, true);                              // ^ 7
    } else if constexpr (M == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);     // odd rows of one copy <-> even rows of the other
        return (lane & 16) ? r[0] : r[1];
    } else {
        static_assert(M == 32, "xor_lane: M must be 1, 2, 4, 8, 16 or 32");
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);     // upper half of one copy <-> lower half of the other
        return (lane & 32) ? r[0] : r[1];
    }
}
#endif

// k_sort.hip
int  sort_padded_size(int n);                 // power of two >= n
int  sort_workgroups(int n);                  // persistent workgroups the sort kernel wants
size_t sort_scratch_bytes(int n);             // device scratch (keys + indices) for all workgroups
struct SortExtras {                        // optional modes of launch_sort_rows (register-blocked bitonic kernel only)
    const int32_t* row_list = nullptr; int n_list = 0;        // sort exactly these rows (instead of the row shard)
    uint8_t* tie_flag = nullptr; unsigned* tie_count = nullptr; unsigned tie_limit = 0;   // flag rows holding equal keys
    uint16_t* tie_bits = nullptr; int64_t ld_bits = 0;        // ... and which sorted elements repeat the key before them
    int max_workgroups = 0;                                    // cap on the grid (0: the default)
    int avoid_xcc = -1; unsigned* row_counter = nullptr;       // leave this XCD to another kernel; rows dealt out by a (zeroed) counter
};
// s_getreg operand of HW_REG_XCC_ID (id 20), bits 3:0: which of the 8 XCDs a wave runs on
static constexpr int GETREG_XCC_ID = 20 | (0 << 6) | (3 << 11);
// The XCD the nn-chain's one-wave kernel claims for itself (k_nnchain.hip), or -1 when it runs spread over all of them
int nnchain_local_xcc(const NNChainOptions& o, int n);
void launch_sort_rows(const double* C, int64_t ldc, const int32_t* order, const int32_t* inv, const double* np_sum,
                      const double* seq_sum, int n, void* scratch, uint16_t* R, int64_t ldr, int row_first, int row_stride,
                      hipStream_t s, const SortExtras& x = SortExtras());
// Rank rows of rows that hold equal keys, from the storage-label sort + its tie bits (k_sort_tied.hip).
void launch_rank_rows_tied(const uint16_t* R_storage, const uint16_t* tie_bits, int64_t ld_bits, const int32_t* order,
                           const int32_t* inv, int n, const int32_t* row_list, int n_list, uint16_t* rank, int64_t ldr,
                           hipStream_t s, int32_t* done = nullptr);     // done: n_list ints of scratch (rows finished by the short-run kernel)
// rank[a][b] = rank_storage[order[a]][order[b]] (rows without equal keys; see k_sort.hip)
void launch_rank_relabel(const uint16_t* rank_storage, uint16_t* rank, int64_t ldr, int n, const int32_t* order, int row_first,
                         int row_stride, hipStream_t s);
size_t sort_radix_scratch_bytes(int n);
void launch_rank_rows_radix(const double* C, int64_t ldc, const int32_t* order, const int32_t* inv, const double* np_sum,
                            const double* seq_sum, int n, void* scratch, uint16_t* rank, int64_t ldr, int row_first,
                            int row_stride, hipStream_t s);   // LSD radix: writes the rank rows directly
void launch_rank_invert(const uint16_t* R, uint16_t* rank, int64_t ldr, int n, int row_first, int row_stride, hipStream_t s,
                        const int32_t* row_list = nullptr, int n_list = 0);
void launch_similarity_row(const double* C, int64_t ldc, const int32_t* order, const double* np_sum,
                           const double* seq_sum, int n, int row, double* out, hipStream_t s);

// k_part2.hip
void launch_p2_select(const double* C, int64_t ldc, const int32_t* sel, int n, double* M2, int64_t ld2, hipStream_t s);
void launch_p2_total(const double* M2, int64_t ld2, int n, double* T, double* total, hipStream_t s);
void launch_p2_score_exact(const double* M2, int64_t ld2, const int32_t* perms, int n_cand, int n_used, double total,
                           double* T, double* work, double* scores, hipStream_t s);
void launch_p2_score(const double* M2, int64_t ld2, const int32_t* perms, int n_cand, int n_used, const double* H,
                     double inv_total_unused, double total, double* scores, hipStream_t s);

void launch_p2_total_perm(const double* M2, int64_t ld2, const int32_t* d_perm, int n, double* T, double* total,
                          hipStream_t s);

// k_part2_search.hip
struct WindowDesc {            // the k <= 8 scaffolds of a window, passed to the kernel by value
    int32_t start[8];          // selection range start of window scaffold j
    int32_t len[8];
    int32_t off[8];            // offset of scaffold j inside the window in the CURRENT arrangement
    uint8_t rev[8];            // current orientation of scaffold j
};
void launch_arr_materialize(const int32_t* packed, int S, const int32_t* scaf_start, const int32_t* scaf_len, int n_arr,
                            int32_t* pos2sel, hipStream_t s);
void launch_p2_base_partial(const double* M2, int64_t ld2, const int32_t* pos2sel, int n_arr, const double* H, int n_tot,
                            int n_blocks, double* out, hipStream_t s);
void launch_p2_insert_delta(const double* M2, int64_t ld2, const int32_t* pos2sel, int n_arr, const int32_t* arr_pos,
                            int S, int new_start, int L, const double* H, int n_base_blocks, double* out, hipStream_t s);
struct WindowBatchEntry {      // one window of a batch (device array)
    WindowDesc w;
    int32_t p0, m;             // first position and number of bins of the window
    int64_t g_off;             // offset of its m x m table in the batch's G buffer
    int32_t c0, pad;           // candidate of the current configuration (identity order, current signs): short lists
};
// (two calls, so that each family - p2_window_G, p2_window_delta - is a timed region of its own)
void launch_p2_window_batch_G(const double* M2, int64_t ld2, const int32_t* pos2sel, int n, const WindowBatchEntry* wb, int n_win,
                              int max_m, const double* H, double* G_all, hipStream_t s);
void launch_p2_window_batch_delta(const double* M2, int64_t ld2, const int32_t* pos2sel, int n, int k,
                                  const WindowBatchEntry* wb, int n_win, int max_m, const int8_t* orders, const uint8_t* orients,
                                  int n_ord, int n_ori, const double* H, const double* G_all, double* delta_all, hipStream_t s);


// k_part2_window.hip: the same scores from placement tables (one pass over the matrix per table, a few look-ups
// per candidate); tables = n_win * window_table_doubles(k) doubles of scratch
int64_t window_table_doubles(int k);
void launch_p2_window_tables(const double* M2, int64_t ld2, const int32_t* pos2sel, int n, int k,
                             const WindowBatchEntry* wb, const WindowBatchEntry* h_wb, int n_win, int max_m, const double* H,
                             double* tables, hipStream_t s);
// ... and the candidates' look-ups in them (the p2_window_delta family)
void launch_p2_window_candidates(int k, int n_win, const int8_t* orders, const uint8_t* orients, int n_ord, int n_ori,
                                 const double* tables, double* delta_all, hipStream_t s);
// The same tables, then only the near-top candidates of every window (the short list of decide_from_delta) without the
// deltas: pass 1 takes each window's largest finite fast score, pass 2 appends the candidates with fast >= thr to
// near[w * cap ...] through the counter count[w] (count[w] > cap: the list overflowed and is incomplete).  whole: k == S
// (fast = delta / total), else fast = cur_fast + (delta - delta[c0]) / total.  part: n_win x window_near_blocks(k, n_ord)
struct NearEntry { int32_t cand, pad; double fast; };
int window_near_blocks(int n_ord);
void launch_p2_window_near(const double* M2, int64_t ld2, const int32_t* pos2sel, int n, int k,
                           const WindowBatchEntry* wb, const WindowBatchEntry* h_wb, int n_win, int max_m, const int8_t* orders,
                           const uint8_t* orients, int n_ord, int n_ori, const double* H, double* tables, int whole, double total,
                           double cur_fast, double floor, double near_top, double* part, int32_t* count, NearEntry* near, int cap,
                           hipStream_t s);

// ---- block sums and the closed-form BASE term, shared by k_part2_search.hip, k_part2_support.hip and k_part2_breaks.hip
__device__ __forceinline__ double wave_sum_s(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ double block_sum_256(double v, double* s_w)
{
    v = wave_sum_s(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// slab `blk` of `n_blk`: rows blk*4 + wave, stepping by 4*n_blk (256-lane workgroup); p: the arrangement in LDS
__device__ __forceinline__ void base_partial_body(const double* __restrict__ M2, int64_t ld2, const int32_t* p, int n_arr,
                                                  const double* __restrict__ H, int n_tot, int blk, int n_blk,
                                                  double* __restrict__ out)
{
    __shared__ double s_w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double hn = H[n_tot - 1];
    double acc = 0.0;
    for (int a = blk * 4 + wave; a < n_arr - 1; a += n_blk * 4) {
        const double* __restrict__ row = M2 + (int64_t)p[a] * ld2;
#pragma unroll 4
        for (int b = a + 1 + lane; b < n_arr; b += 64) acc += row[p[b]] * (hn - H[b - a - 1]);
    }
    double sum = block_sum_256(acc, s_w);
    if (threadIdx.x == 0) out[0] = sum;
}

// ---- the pick of a table record, shared by k_part2_support.hip and k_part2_breaks.hip ("The pick").
// A 256-lane workgroup has just written scores[0 .. n_cand), thread tid the entries tid, tid + 256, ...; every thread
// reads back only what it wrote.  Among the candidates i with counts(i) and a finite score: best[0] = the first maximum
// (the lowest index among equals), best[1] = how many lie within near_top of it, relative; (-1, 0) when nothing competes.
// The host restates this rule as support_summary / break_summary (orderGenome.py).  10 barriers.
template <typename Counts>
__device__ __forceinline__ void pick_first_max_256(int tid, int n_cand, const double* scores, int32_t* best,
                                                   double near_top, Counts counts)
{
    __shared__ double s_val[256];
    __shared__ int s_idx[256], s_cnt;
    double mx = -__builtin_inf();
    int at = 0x7fffffff;
    for (int i = tid; i < n_cand; i += 256) {
        const double v = scores[i];
        if (counts(i) && isfinite(v) && v > mx) { mx = v; at = i; }   // ascending i: the first of equals
    }
    s_val[tid] = mx; s_idx[tid] = at;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) {
            const double o = s_val[tid + w];
            const int oi = s_idx[tid + w];
            if (o > s_val[tid] || (o == s_val[tid] && oi < s_idx[tid])) { s_val[tid] = o; s_idx[tid] = oi; }
        }
        __syncthreads();
    }
    const double top = s_val[0];
    const int first = s_idx[0];
    if (first == 0x7fffffff) {                           // nothing competes, or nothing finite
        if (tid == 0) { best[0] = -1; best[1] = 0; }
        return;
    }
    const double thr = top - fabs(top) * near_top;
    int near = 0;
    for (int i = tid; i < n_cand; i += 256) {
        const double v = scores[i];
        near += counts(i) && isfinite(v) && v >= thr;
    }
    if (near) atomicAdd(&s_cnt, near);
    __syncthreads();
    if (tid == 0) { best[0] = first; best[1] = s_cnt; }
}

// Lock-step insertion (k_part2_insert.hip): orderRemainderScaffolds for several chromosomes at once, every
// decision taken on the device.  One InsStep per (step, chromosome), built by the host in advance.
static constexpr int INS_MAXC = 8;       // candidates re-scored literally per step; more -> the host decides that step
struct InsState {
    int32_t fail;                        // -1, or the first step the device could not decide
    int32_t n_short;                     // short-listed candidates of the current step
    int32_t direct, pad;                 // 1: the step has ONE candidate near the top - slot 0 is taken without a literal score
    int32_t gap[INS_MAXC], rev[INS_MAXC], idx[INS_MAXC];   // idx = position in the reference's enumeration
    double total;                        // literal total of the step (OG:343), formed when a literal pass runs
    double lit[INS_MAXC];                // literal scores of the short list
};
struct InsLog { int32_t gap, rev; double best; int32_t n_short, pad; };
struct InsStep {
    const double* M2; const double* H; int64_t ld2;
    const int32_t* pos_cur; int32_t* pos_nxt;            // arrangement as bin order (ping-pong)
    const int32_t* packed_cur; int32_t* packed_nxt;       // [S ids][S+1 prefix positions][S reversed flags]
    double *T_total, *T_cand, *work, *partial;
    InsState* st; InsLog* log;                            // log: this step's entry
    int32_t n_arr, S, L, new_start, new_id, active, step, last;   // last: the job's final step (its score is returned)
};
// k_part2.hip / k_part2_search.hip / k_part2_insert.hip: one launch serves all chromosomes (blockIdx.y)
void launch_insb_reset(const InsStep* steps, int n_chrom, hipStream_t s);
void launch_insb_fast(const InsStep* steps, int n_chrom, int max_S, int max_n_arr, int n_base_blocks, hipStream_t s);
void launch_insb_shortlist(const InsStep* steps, int n_chrom, int max_S, int max_n_arr, int n_base_blocks, double near_top,
                           int max_c, hipStream_t s);
void launch_insb_diag_cand(const InsStep* steps, int n_chrom, int max_n_used, hipStream_t s);
void launch_insb_cost(const InsStep* steps, int n_chrom, int max_n_used, hipStream_t s);
void launch_insb_apply(const InsStep* steps, int n_chrom, int max_n_used, hipStream_t s);

// k_part2_support.hip: placement support (hicmi_p2_support_multi).  One record per (chromosome, left-out scaffold j):
// the insertion step "A without j, j put back", read through A's own arrays.
static constexpr int SUP_BASE_SLABS = 64;     // partial sums of a record's BASE term
static constexpr int SUP_MAX_S = 4096;        // scaffolds per chromosome (the table has 2 S^2 entries)
struct SupRec {
    const double* M2; const double* H; int64_t ld2;
    const int32_t* pos;                       // A as bin order, n entries
    const int32_t* arr_pos;                   // prefix positions of A's S scaffolds, S + 1 entries
    double* partial;                          // [SUP_BASE_SLABS BASE slabs][n - L row values][2 S CROSS terms]
    double* scores;                           // out: score(j, g, r) at [2 g + r]
    int32_t* best;                            // out: the pick (pick_first_max_256) over sup_counts
    double total;
    int32_t n, S, j, start, L, cur_rev;       // start, L: j's range of the selection; cur_rev: its orientation in A
};
void launch_sup(const SupRec* recs, int n_rec, int max_S, int max_n, double near_top, hipStream_t s);

// k_part2_breaks.hip: break support (hicmi_p2_breaks_multi).  One record per (chromosome, scaffold j of at least 2 bins):
// j cut between two of its bins, the two pieces swapped and / or reversed in place.
static constexpr int BRK_BASE_SLABS = 64;     // partial sums of a chromosome's BASE term
struct BrkRec {
    const double* M2; const double* H; int64_t ld2;
    const int32_t* pos;                       // A as bin order, n entries
    double* X;                                // scratch: L x L, [bin of the block as laid down][position inside the block]
    double* pq;                               // scratch: [L - 1 cuts][3 P x Q sums]
    double* base;                             // the chromosome's BRK_BASE_SLABS BASE slabs (one area for all its records)
    double* scores;                           // out: score(p, k) at [8 (p - 1) + k]
    int32_t* best;                            // out: the pick (pick_first_max_256) over brk_counts
    double total;
    int64_t wg0;                              // first workgroup of this record in k_brk_tables
    int32_t n, B, L, min_piece;               // B: first position of j in A
    int32_t n_base, pad;                      // BRK_BASE_SLABS for a chromosome's first record (it forms the slabs), else 0
};
void launch_brk(const BrkRec* recs, int n_rec, int64_t n_wg, double near_top, hipStream_t s);

// k_part2_invert.hip: inversion support (hicmi_p2_inversions_multi).  One record per (chromosome, left end i): the
// scaffolds i ... j of the arrangement reversed and flipped, for every right end j = i ... i + n_j - 1.
static constexpr int INV_BASE_SLABS = 64;     // partial sums of a chromosome's BASE term
static constexpr int INV_MAX_S = 4096;        // scaffolds per chromosome (the table has S^2 entries)
static constexpr double INV_MAX_WORK = 1e13;  // matrix elements read by one call: sum of len * (n - len) over its candidates
struct InvRec {
    const double* M2; const double* H; int64_t ld2;
    const int32_t* pos;                       // A as bin order, n entries
    const int32_t* arr_pos;                   // prefix positions of A's S scaffolds, S + 1 entries
    double* base;                             // the chromosome's INV_BASE_SLABS BASE slabs (one area for all its records)
    double* scores;                           // out: row i of the S x S table, score(i, j) at [j]
    int32_t* best;                            // out: the pick (pick_first_max_256) over inv_counts
    double total;
    int64_t wg0;                              // first workgroup of this record in k_inv_tables
    int32_t n, S, i, n_j;                     // n_j: right ends computed, j = i ... i + n_j - 1 (max_span cuts it short)
    int32_t max_span, n_base;                 // n_base: INV_BASE_SLABS for a chromosome's first record (it forms the slabs), else 0
};
void launch_inv(const InvRec* recs, int n_rec, int64_t n_wg, double near_top, hipStream_t s);

// k_group_support.hip: group support (hicmi_group_sums).  rows: the grouped rows sorted by group, ascending inside a
// group; chunks[c]: rows[row0 .. row0 + cnt) with cnt <= GS_CHUNK, all of one group; group_chunk0[g] .. [g + 1]: the
// chunks of group g; sbins / soff: the bins sorted by scaffold.  partial: n_chunks x n, binsum: n x G, scafsum: S x G.
static constexpr int GS_CHUNK = 64;           // member rows per chunk: part of the definition
struct GsChunk { int32_t row0, cnt, group, pad; };
void launch_group_sums(const double* C, int64_t ld, int n, int G, int S, const int32_t* rows, const GsChunk* chunks,
                       int n_chunks, const int32_t* group_chunk0, const int32_t* scaf, const int32_t* sbins,
                       const int32_t* soff, double* partial, double* binsum, double* scafsum, bool plain, hipStream_t s);

// k_junctions.hip: junction support (hicmi_junction_sums).  bins: the bin order of every chromosome, one
// after the other (matrix indices); a record's two sides are views of it; w[d] = 1.0 / d for d = 1 .. the largest
// lenA + lenB - 1 of the call (w[0] unused); partial: one double per workgroup; sums: one per record.
static constexpr int JN_SLAB_ROWS = 64;       // rows of A per workgroup: part of the summation order
struct JnRec {
    int64_t wg0;                              // first workgroup of this record in k_junctions_partial
    int32_t startA, stepA, lenA;              // side entry k = bins[start + k * step], step = +1 or -1
    int32_t startB, stepB, lenB;
    int32_t n_slabs, pad;                     // ceil(lenA / JN_SLAB_ROWS)
};
void launch_junction_sums(const double* C, int64_t ld, const int32_t* bins, const JnRec* recs, int n_rec, int64_t n_wg,
                          const double* w, double* partial, double* sums, bool plain, hipStream_t s);

// k_ice.hip: ICE balancing of a raw map (hicmi_ice_balance).  st: [mean0, last c]; rec: (delta, c) per
// iteration; u == nullptr in the vector steps: the in-place path.
void launch_ice_fill(double* v, int n, double value, hipStream_t s);
void launch_ice_rowdot(const double* C, int64_t ld, int n, const double* u, double* y, hipStream_t s);
void launch_ice_vec_b(int n, const double* y, double* u, double* bias, double* prev, double* sums, double* st,
                      double* rec, int it, int first, hipStream_t s);
void launch_ice_vec_a(int n, const double* sums, double* bias, double* u, double* d, hipStream_t s);
void launch_ice_apply(double* X, int64_t ld, int n, const double* u, hipStream_t s);
void launch_ice_scale(double* X, int64_t ld, int n, const double* d, const double* st, int by_c, hipStream_t s);
void launch_ice_mask(double* X, int64_t ld, int n, const uint8_t* mask, hipStream_t s);

// k_rebin.hip: a raw map summed to a coarser resolution (hicmi_rebin).  group_start: m + 1 entries;
// chunk_first[c], c = 0 .. ceil(n / REBIN_CHUNK): the coarse columns with group_start[J + 1] <= c * REBIN_CHUNK.  R: m x m.
static constexpr int REBIN_MAX_WIDTH = 64;    // fine bins per coarse bin
static constexpr int REBIN_CHUNK = 1024;      // fine columns a workgroup of k_rebin holds column sums of at a time
void launch_rebin(const double* C, int64_t ld, int n, const int32_t* group_start, const int32_t* chunk_first, int m,
                  double* R, bool plain, hipStream_t s);

// k_buildmap.hip: a raw map counted from read pairs (hicmi_map_*, hicmi_build_maps).  The four pair arrays
// and first_bin (n_grid entries) are device memory; counts: m x m unsigned 64-bit cells, of which the upper triangle is
// counted; launch_buildmap_finish turns them in place into the symmetric matrix of doubles.  With lift tables
// (lift.seq != nullptr, device pointers) every end is lifted to its assembled sequence first and first_bin
// describes the sequences.  launch_pair_stats adds the statistics of the pairs to out[256 + 2 n_seq + 1]: the decay
// histogram, cis and trans per sequence, the unlifted pairs.
static constexpr int BUILDMAP_SLICE = 2048;   // pairs a workgroup of k_buildmap_combine brings together
static constexpr int BUILDMAP_SLOTS = 4096;   // slots of its hash table in LDS (12 bytes each)
static constexpr int PAIRSTATS_SLICE = 1024;  // pairs a workgroup of k_pair_stats brings together: up to two keys each
static constexpr int PAIRSTATS_SLOT_BITS = 12;
static constexpr int PAIRSTATS_SLOTS = 1 << PAIRSTATS_SLOT_BITS;   // slots of its table in LDS (8 bytes each)
void launch_buildmap_add(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                         const int32_t* first_bin, int n_grid, int64_t r, int m, void* counts, bool plain, const LiftTables& lift,
                         hipStream_t s);
void launch_pair_stats(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       const LiftTables& lift, void* out, hipStream_t s);
void launch_buildmap_finish(void* cells, int m, hipStream_t s);

// k_spans.hip: spanning depth from read pairs (hicmi_span_*).  marks: n_cells unsigned 64-bit cells, +1 and
// -1 (two's complement) per marking pair; counters: the five kinds of pairs (SpanKind).  launch_span_scan: out = inclusive
// prefix sum of in (n elements, in != out), tile_sums: span_scan_tiles(n) elements of scratch.  launch_span_pick: four
// integers (slot, D, Lsum, Rsum) per record (lo, hi, q0, q1); everything is device memory.
static constexpr int SPAN_SLICE = 2048;        // pairs a workgroup of the combining k_span_mark brings together: two marks each
static constexpr int SPAN_SLOT_BITS = 11;
static constexpr int SPAN_SLOTS = 1 << SPAN_SLOT_BITS;   // slots of its table in LDS (8 bytes each); a slice can need twice as many
static constexpr int SPAN_PROBES = 8;          // a mark that finds no room within so many probes is added directly
static constexpr int SPAN_SCAN_ITEMS = 8;      // elements a thread of the scan takes in a row
static constexpr int SPAN_SCAN_TILE = 2048;    // elements of one workgroup of k_span_tile_sums and k_span_scan_add
static constexpr int SPAN_SCAN_WIDTH = 1024;   // tile sums the one workgroup of k_span_scan_tiles takes at a time
void launch_span_mark(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                      const LiftTables& lift, const SpanGrid& grid, void* marks, void* counters, bool plain, hipStream_t s);
int64_t span_scan_tiles(int64_t n);
void launch_span_scan(const void* in, void* out, int64_t n, void* tile_sums, hipStream_t s);
void launch_span_pick(const void* depth, const void* depth_sums, int64_t n_cells, int64_t flank, const int64_t* recs, int64_t n_rec,
                      int64_t* picks, hipStream_t s);

// k_ends.hip: read-pair links between the ends of ordered scaffolds (hicmi_ends_*).  table: n_table =
// placed x reach x 4 unsigned 64-bit counters, +1 per linked pair; counters: the six kinds of pairs (EndsKind); everything is
// device memory.
static constexpr int ENDS_SLICE = 2048;        // pairs a workgroup of the combining k_ends_count brings together: one counter each
static constexpr int ENDS_SLOT_BITS = 10;
static constexpr int ENDS_SLOTS = 1 << ENDS_SLOT_BITS;   // slots of its table in LDS (8 bytes each); a slice can need twice as many
static constexpr int ENDS_PROBES = 8;          // a pair that finds no room within so many probes is added directly
void launch_ends_count(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       const LiftTables& lift, const EndsGrid& grid, int64_t n_table, void* table, void* counters, bool plain,
                       hipStream_t s);

// k_anchor.hip: read-pair links between the scaffolds an ordering leaves out and the placed ones (hicmi_anchor_*; DESIGN.md
// 9q).  table: n_table unsigned 64-bit counters, the blocks of the candidates (anchor.h), +1 per anchored pair; counters:
// the six kinds of pairs (AnchorKind); everything is device memory.
static constexpr int ANCHOR_SLICE = 2048;      // pairs a workgroup of the combining k_anchor_count brings together: one counter each
static constexpr int ANCHOR_SLOT_BITS = 10;
static constexpr int ANCHOR_SLOTS = 1 << ANCHOR_SLOT_BITS;   // slots of its table in LDS (8 bytes each); a slice can need twice as many
static constexpr int ANCHOR_PROBES = 8;        // a pair that finds no room within so many probes is added directly
void launch_anchor_count(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                         const LiftTables& lift, const AnchorGrid& grid, int64_t n_table, void* table, void* counters, bool plain,
                         hipStream_t s);

// k_seats.hip: read-pair links of every placed scaffold with the chromosomes and with the end zones of the scaffolds of its
// own chromosome (hicmi_seats_resident).  table: n_table unsigned 64-bit counters, the blocks of the placed
// scaffolds (seats.h), up to four adds per pair; counters: the five kinds of pairs (SeatsKind); everything is device memory.
static constexpr int SEATS_SLICE = 4096;       // pairs a workgroup of the combining k_seats_count brings together: up to four counters each
static constexpr int SEATS_SLOT_BITS = 12;
static constexpr int SEATS_SLOTS = 1 << SEATS_SLOT_BITS;     // slots of its table in LDS (8 bytes each, 32 KB); a slice can need four times as many
static constexpr int SEATS_PROBES = 8;         // an add that finds no room within so many probes goes to global memory directly
void launch_seats_count(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                        const LiftTables& lift, const SeatsGrid& grid, int64_t n_table, void* table, void* counters, bool plain,
                        hipStream_t s);

// k_links.hip: the end-link graph of all scaffolds from the resident pair store (hicmi_links_resident).  The
// find-or-insert table: keys (LINKS_EMPTY: free) and counts of cap = 2^bits slots, and behind them LINKS_EXTRAS unsigned
// 64-bit integers: the two kinds of pairs (LinksKind), a flag (bit 0: an insert found the table full, bit 1: a record
// found no room) and the number of records k_links_compact wrote; everything is device memory, zeroed by the caller but for
// the keys, which start out as LINKS_EMPTY.
static constexpr int LINKS_SLICE = 8192;       // pairs a workgroup of the combining k_links_count brings together
static constexpr int LINKS_SLOT_BITS = 11;
static constexpr int LINKS_SLOTS = 1 << LINKS_SLOT_BITS;     // slots of its table in LDS (12 bytes each, 24 KB)
static constexpr int LINKS_PROBES = 8;         // an add that finds no room within so many probes goes to the global table directly
static constexpr int LINKS_COMPACT_SLICE = 4096;   // slots a workgroup of k_links_compact takes: one bump of the record count each
static constexpr int LINKS_FLAG = LINKS_COUNTERS, LINKS_RECORDS = LINKS_COUNTERS + 1, LINKS_EXTRAS = LINKS_COUNTERS + 2;
struct LinksTable {
    unsigned long long* keys = nullptr;
    unsigned long long* counts = nullptr;
    unsigned long long* extras = nullptr;
    int64_t cap = 0;
    int bits = 0;
};
void launch_links_count(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                        const int64_t* scaf_size, int64_t n_scaf, int64_t window, const LinksTable& table, bool plain, hipStream_t s);
// The count on lifted ends (hicmi_links_lifted): the same table with LINKS_LIFTED_EXTRAS integers behind the
// counts.  The first LINKS_EXTRAS are what they are above, so links_add_global and k_links_compact find the flag and the
// number of records where they look for them; the counters of the kinds INSIDE and UNLIFTED follow.  seq_size: n_seq sizes
// of the sequences of `lift`, device memory.
static constexpr int LINKS_LIFTED_EXTRAS = LINKS_EXTRAS + (LINKS_LIFTED_COUNTERS - LINKS_COUNTERS);
constexpr int links_lifted_extra(int kind) { return kind < LINKS_COUNTERS ? kind : LINKS_EXTRAS + (kind - LINKS_COUNTERS); }
void launch_links_count_lifted(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                               const LiftTables& lift, const int64_t* seq_size, int64_t window, const LinksTable& table, bool plain,
                               hipStream_t s);
// the used slots as rec_cap (key, count) records at the most, in no order
void launch_links_compact(const LinksTable& table, void* rec_key, void* rec_cnt, int64_t rec_cap, hipStream_t s);

// k_pairs.hip: the resident pair store (hicmi_pairs_*).  A chunk of n pairs on the device is compacted into
// the store: the kept pairs (pairs.h) are appended from *length on, which is advanced, and the others add to intra[n_scaf].
// work: pairs_keep_blocks(n) 64-bit integers of the default form; everything is device memory, and the caller has made room
// for *length + n pairs.
static constexpr int PAIRS_SLICE = 2048;       // pairs a workgroup of the stable k_pairs_keep compacts: one offset per workgroup
static constexpr int PAIRS_SLOT_BITS = 8;
static constexpr int PAIRS_SLOTS = 1 << PAIRS_SLOT_BITS;   // slots of the intra table in LDS (8 bytes each): scaffolds of a slice
static constexpr int PAIRS_PROBES = 8;         // an intra pair that finds no room within so many probes is added directly
struct PairStore { int32_t* scaf_a = nullptr; int64_t* pos_a = nullptr; int32_t* scaf_b = nullptr; int64_t* pos_b = nullptr; int64_t cap = 0; };
int64_t pairs_keep_blocks(int64_t n);
void launch_pairs_keep(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       int64_t n_scaf, const PairStore& store, void* length, void* intra, void* work, bool plain, hipStream_t s);

// k_split.hip: a chunk of pairs moved in place from scaffolds to the pieces they are cut into (hicmi_split_*),
// each pair adding to counters[4 n_piece] = [within][sibling][other][mark] of its pieces; everything is device memory.
static constexpr int SPLIT_SLICE = 2048;       // pairs a workgroup of the combining k_split_pairs takes at a time: up to four counters each
static constexpr int SPLIT_SLOT_BITS = 11;
static constexpr int SPLIT_SLOTS = 1 << SPLIT_SLOT_BITS;   // slots of its table in LDS (8 bytes each), kept over all its slices
static constexpr int SPLIT_PROBES = 8;         // a contribution that finds no room within so many probes is added directly
static constexpr int SPLIT_MAX_BLOCKS = 1024;  // workgroups of the grid-stride loop: four per compute unit of an MI355X
void launch_split_pairs(int32_t* scaf_a, int64_t* pos_a, int32_t* scaf_b, int64_t* pos_b, int64_t n, const SplitTables& tables,
                        void* counters, bool plain, hipStream_t s);

// k_plot.hip
void launch_plot_select(const double* C, int64_t ldc, const double* np_sum, const double* seq_sum, int kind,
                        const int32_t* order, int n_sel, int n_targets, struct SelectState* d_state, unsigned int* d_hist,
                        hipStream_t s);
size_t plot_select_state_bytes();
size_t plot_select_hist_bytes();
int plot_select_max_targets();
void plot_select_fill(void* host_state, const unsigned long long* ranks, int n_targets);
double plot_select_value(const void* host_state, int t);
void launch_plot_downsample(const double* C, int64_t ldc, const double* np_sum, const double* seq_sum, int kind,
                            const int32_t* order, int n_sel, int px, double* out, hipStream_t s);

// k_hmm.hip: the HMM boundary finder (S2C:730-942).  Model parameters live in one fp64 buffer: blocks of 2 x D
// (state-major) at offset HMM_P_* x D, then HMM_S_COUNT scalars at HMM_P_SCALARS x D.
enum { HMM_P_MEAN = 0, HMM_P_VAR = 2, HMM_P_MOV = 4, HMM_P_IV = 6, HMM_P_LOGV = 8, HMM_P_MU2V = 10, HMM_P_SCALARS = 12 };
enum { HMM_S_CONST = 0, HMM_S_A = 2, HMM_S_LOGA = 6, HMM_S_PI = 10, HMM_S_LOGPI = 12, HMM_S_XI = 14, HMM_S_POST = 18,
       HMM_S_COUNT = 32 };
int  hmm_col_chunks(int T, int D);                       // row chunks of a column pass (partials: chunks x 4 x D doubles)
// the row chunking of a column pass: rows per chunk and the chunks that hold rows
__host__ __device__ inline void hmm_col_shape(int T, int R, int& rows_per, int& Rr)
{
    rows_per = (T + R - 1) / R;
    Rr = (T + rows_per - 1) / rows_per;
}
// One problem of hicmi_hmm_dist2_multi / hicmi_hmm_kmeans_multi: a view (T x D, leading dimension ld) of a resident X,
// its nc seed rows, and its own work areas - centers (2 D), combined sums (2 D), column partials (Rr x 2 x D), out
// (dist2: nc x T distances; k-means: T per-row minimum distances), labels (two generations, 2 T).
struct HmmKmProb {
    const double* X; int64_t ld; int T, D;
    int nc, rows_per, Rr, max_iter;
    int64_t rows[2];
    double tol;
    double *cen, *sums, *part, *out;
    int32_t* lab;
};
enum { HMM_KM_LLOYD = 0, HMM_KM_FINAL = 1, HMM_KM_SUM = 2, HMM_KM_DONE = 3 };
// the device-side state of one k-means problem: phase, which label generation is current, iterations run, the
// iteration's counters (labels changed, rows with label 1), the inertia once done
struct HmmKmState { int phase, cur, it, strict, changed, n1; double inertia; };
void launch_hmm_obs(const double* C, int64_t ldc, const int32_t* order, const double* np_sum, const double* seq_sum,
                    int c, int T, int D, double* X, hipStream_t s);
void launch_hmm_colsum(int mode, const double* X, int64_t ld, int T, int D, const double* shift, const int32_t* labels,
                       const double* g, double* part, double* out, hipStream_t s);
void launch_hmm_dist2(const double* X, int64_t ld, int T, int D, const double* cen, int nc, double* dist, hipStream_t s);
void launch_hmm_assign(const double* X, int64_t ld, int T, int D, const double* cen, const int32_t* old_labels,
                       int32_t* labels, double* mind, int* st, hipStream_t s);
void launch_hmm_center_update(const double* sums, int T, int D, const int* st, double* cen, double* shift_out, hipStream_t s);
void launch_hmm_sum(const double* v, int n, double* out, hipStream_t s);
void launch_hmm_params(const double* sums, int D, int from_sums, double* P, hipStream_t s);
void launch_hmm_emission(const double* X, int64_t ld, int T, int D, const double* P, double* L, hipStream_t s);
void launch_hmm_fb(const double* L, int T, double* P, int D, double* alpha, double* beta, double* gam, double* hist, int it,
                   hipStream_t s);
void launch_hmm_viterbi(const double* L, int T, const double* P, int D, uint8_t* bt, int32_t* states, hipStream_t s);
void launch_hmm_multi_seed(const HmmKmProb* pr, HmmKmState* st, int n_prob, int max_rows, int kmeans, hipStream_t s);
void launch_hmm_dist2_multi(const HmmKmProb* pr, int n_prob, int max_T, hipStream_t s);
// one Lloyd step of every live problem: assignment, label-masked column sums, combine, center update + stop rule
void launch_hmm_kmeans_multi_step(const HmmKmProb* pr, HmmKmState* st, int* done, int n_prob, int max_T, int max_items,
                                  int max_2d, hipStream_t s);

// k_louvain.hip: level 0 of the Louvain tail (S2C:239-349, modularity.py).  The graph is m x m, leading dimension m.
static constexpr int LOUVAIN_MAX_M = 16384;
static constexpr int LOUVAIN_MAX_ROUNDS = 1024;
// per-round work arrays of the level-0 sweep: 4 fp64 and 8 int32 arrays of m
__host__ __device__ inline size_t louvain_round_bytes(int m) { return (size_t)m * (4 * sizeof(double) + 8 * sizeof(int)); }
int  louvain_level0_lds_max();                            // the most of them one workgroup keeps in LDS
void launch_louvain_graph(const double* C, int64_t ldc, const int32_t* rows, const double* np_sum, const double* seq_sum, int m,
                          double* A, hipStream_t s);
void launch_louvain_status(const double* A, int m, double* diag, double* rowsum, double* chunk, double* dsum, double* gdeg,
                           double* total, hipStream_t s);
void launch_louvain_level0(const double* A, int m, const double* gdeg, const double* loops, const double* total, int rounds,
                           const uint64_t* st_in, int32_t* n2c_out, uint64_t* st_out, int32_t* info, double* deg_out,
                           double* int_out, unsigned char* scratch, hipStream_t s);
void launch_louvain_induced(const double* A, int m, const int32_t* members, const int32_t* moff, int k, double* rowagg,
                            double* B, hipStream_t s);
void launch_louvain_score(const double* A, int m, const int32_t* parts, int rounds, const double* gdeg, const double* total,
                          double* same, double* acc, double* q, hipStream_t s);

}  // namespace hicmi
