// api.hip - the C ABI of libhicmi.so (include/hicmi.h): context, device buffers, stage drivers,
// and the small host-side pieces of SciPy's linkage post-processing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <functional>
#include <chrono>
#include <vector>

#include "../../include/hicmi.h"
#include "hicmi_internal.h"
#include "devbuf.h"
#include "hyper.h"

using namespace hicmi;

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace hicmi { int set_error(int code, const char* msg) { return fail(code, "%s", msg); } }

#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return fail(HICMI_EHIP, "%s: %s", #expr, hipGetErrorString(_e));     \
    } while (0)

enum Family { F_ROW_SUMS, F_BUILD_W, F_NNCHAIN, F_SORT, F_RANK_INVERT, F_CUT_COUNT, F_HYPER_FLAGS, F_P2_SELECT,
              F_P2_TOTAL, F_P2_SCORE, F_P2_EXACT, F_P2_INSERT, F_P2_WINDOW_G, F_P2_WINDOW_DELTA, F_PLOT, F_PRESORT, F_RANK_RELABEL,
              F_RANK_TIED, F_P2_WINDOW_FLOPS, F_COUNT };
static const char* kFamilyNames[F_COUNT] = {"row_sums", "build_w", "nnchain", "sort_rows", "rank_invert",
                                            "cut_count", "hyper_flags", "p2_select", "p2_total", "p2_score",
                                            "p2_score_exact", "p2_score_insert", "p2_window_G", "p2_window_delta", "plot",
                                            "presort_rows", "rank_relabel", "rank_rows_tied",
                                            "p2_window_G_flops"};      // (its "bytes" are FLOPS of the window tables' GEMM)

constexpr int kBaseSlabs = 256;                        // partial sums of the closed-form BASE term (one slab per workgroup)

struct TimedRegion { int fam; hipEvent_t a, b; };

// The context.  Members are destroyed in reverse order of declaration, and hicmi_destroy relies on it: every buffer
// below the handles is freed first, then the timing events, ev_join / ev_fork, stream2 and at last the stream.
template <typename H, hipError_t (*Destroy)(H)>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(const Handle&) = delete;
    ~Handle() { if (h) (void)Destroy(h); }
    operator H() const { return h; }
};
using StreamHandle = Handle<hipStream_t, hipStreamDestroy>;
using EventHandle = Handle<hipEvent_t, hipEventDestroy>;
struct TimingEvents {
    std::vector<TimedRegion> regions;
    std::vector<hipEvent_t> pool;
    TimingEvents() = default;
    TimingEvents(const TimingEvents&) = delete;
    ~TimingEvents()
    {
        for (auto& r : regions) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

struct hicmi_ctx {
    int device = 0;
    StreamHandle stream;
    // pre-sort: the rank rows in storage labels, computed on a second stream while the nn-chain runs (hicmi_upgma)
    StreamHandle stream2; EventHandle ev_fork, ev_join;
    TimingEvents tev;
    int probed_xcc = 0;                  // the lowest XCD id of the device (nnchain_probe_xcc): the nn-chain's default XCD
    // contacts: dC is the caller's matrix (adopted, own_c false) or c_own's memory
    int64_t n = 0, ldc = 0;
    double* dC = nullptr;
    bool own_c = false;
    DevBuf<double> c_own;
    DevBuf<double> d_np, d_seq;
    bool have_sums = false;
    // row shard (one map over several GPUs): this context sorts / counts only rows first, first + stride, ...
    int64_t shard_first = 0, shard_stride = 1;
    // upgma: one group, w_rows x ldw
    DevBuf<double> dW, dW2; int64_t ldw = 0; int64_t w_rows = 0;
    DevBuf<unsigned char> d_size;        // the nn-chain's workspace (nnchain_workspace_bytes)
    DevBuf<int> d_chain, d_status;
    DevBuf<double> d_zraw;
    std::vector<double> zraw;
    // rank matrix: dRank and d_order are one group, r_rows x ldr
    DevBuf<int32_t> d_order;
    DevBuf<uint16_t> dR, dRank; int64_t ldr = 0; int64_t r_rows = 0;
    DevBuf<unsigned char> d_sort_scratch;
    bool have_rank = false;
    // pre-sort buffers: one group
    DevBuf<uint16_t> dRankS;
    DevBuf<int32_t> d_ident;
    DevBuf<unsigned char> d_ties;        // [count of flagged rows, 16 bytes][one flag per storage row]
    DevBuf<uint16_t> d_tie_bits; int64_t ld_bits = 0;   // per storage row: "same key as the element before"
    DevBuf<int32_t> d_row_list;          // the list + one flag per listed row
    int64_t scan_first_batch = 0, scan_last_improved = 0;   // hicmi_p2_scan_all: the first batch size of the next round
    int64_t presort_tied_rows = 0;                        // ... and how many rows it re-sorted because they hold equal keys
    int presort_used = 0;                                 // last hicmi_rank_matrix: 0 sorted itself, 1 relabelled the pre-sort, 2 pre-sort discarded (ties)
    int64_t presort_n = 0;                                // > 0: dRankS holds the rows of the current n x n matrix
    bool presort_dealt = false;                           // its rows were dealt out by a counter (workgroups on the chain's XCD left)
    // cut scan
    DevBuf<int32_t> d_x; DevBuf<uint8_t> d_sig;
    DevBuf<unsigned char> d_scan_multi;  // device-driven scan loops: state records + lists
    int64_t cached_start = -1;
    DevBuf<double> d_tmp;
    // part 2
    DevBuf<double> dM2; int64_t n2 = 0, ld2 = 0;
    DevBuf<int32_t> d_sel;
    DevBuf<double> d_H;
    DevBuf<int32_t> d_perms;
    DevBuf<double> d_scores;
    DevBuf<double> d_partial;
    DevBuf<double> d_T;
    // part 2 search state: layout (scaffold ranges of the selection), arrangement, window tables
    DevBuf<int32_t> d_scaf_start, d_scaf_len; int64_t n_scaf = 0;
    std::vector<int32_t> h_scaf_start, h_scaf_len;
    DevBuf<int32_t> d_arr_packed;        // [S ids][S+1 positions][S reversed flags]
    std::vector<int32_t> h_arr_packed;
    std::vector<int32_t> h_arr_id, h_arr_pos; std::vector<uint8_t> h_arr_rev;
    DevBuf<int32_t> d_pos2sel; int64_t n_arr = 0;
    DevBuf<int8_t> d_orders; DevBuf<uint8_t> d_orients;
    int tab_k = 0; int64_t n_orders = 0, n_orients = 0;
    std::vector<int8_t> h_orders; std::vector<uint8_t> h_orients;
    std::vector<int32_t> h_pos2sel;                              // host mirror of the arrangement's bin order
    uint64_t arr_version = 0;                                    // bumped by every hicmi_p2_set_arrangement
    uint64_t cur_lit_version = ~0ull; double cur_lit_total = 0.0, cur_lit_value = 0.0;   // literal score of the arrangement itself
    double cache_total = 0.0; bool cache_valid = false;          // literal scores under one total, keyed by bin order
    std::unordered_map<std::string, double> exact_cache;
    DevBuf<double> d_G;
    DevBuf<double> d_delta;
    DevBuf<WindowBatchEntry> d_wb;
    // short lists of wide windows decided on the device (HICMI_P2_DEVICE_DECIDE, read at creation): windows of at least
    // near_min_k scaffolds; [pass-1 partials][per-window counters][NearEntry lists]
    int near_min_k = 7;
    DevBuf<unsigned char> d_wnear;
    // device-decided insertion (k_part2_insert.hip): second arrangement buffers (ping-pong) and work areas
    DevBuf<int32_t> d_arr_packed2;
    DevBuf<int32_t> d_pos2sel2;
    DevBuf<double> d_ins_T;
    DevBuf<double> d_ins_partial;
    DevBuf<unsigned char> d_ins_blob;    // per job: [InsState][InsLog x steps]
    DevBuf<InsStep> d_ins_steps;         // [step][job] records of a lock-step queue
    DevBuf<SupRec> d_sup_recs;           // hicmi_p2_support_multi: (chromosome, left-out scaffold) records
    DevBuf<BrkRec> d_brk_recs;           // hicmi_p2_breaks_multi: (chromosome, scaffold of 2+ bins) records
    DevBuf<InvRec> d_inv_recs;           // hicmi_p2_inversions_multi: (chromosome, left end) records
    // group support (k_group_support.hip): the member lists of a call, and its partials + the two tables
    DevBuf<int32_t> d_gs_lists;
    DevBuf<double> d_gs_sums;
    // junction support (k_junctions.hip): [records][bin order] of a call, and its [weights][partials][sums]
    DevBuf<unsigned char> d_jn_lists;
    DevBuf<double> d_jn_sums;
    // ICE balancing (k_ice.hip): [y][u][bias][bias_prev][s][d][ones] of n each, [mean0, c], (delta, c) per iteration; the mask
    DevBuf<double> d_ice;
    DevBuf<uint8_t> d_ice_mask;
    // HMM boundary finder (k_hmm.hip): resident observation matrices, one per slot (T x ld, columns [0, D) in use);
    // the selected slot's view is mirrored in d_hx / hmm_T / hmm_ld / hmm_D for the single-problem entry points.  The
    // work areas are sized for the largest slot built
    struct HmmSlot { DevBuf<double> d_x; int64_t T = 0, ld = 0, D = 0; };
    HmmSlot hslot[HICMI_HMM_MAX_SLOTS]; int hcur = 0;
    double* d_hx = nullptr; int64_t hmm_T = 0, hmm_ld = 0, hmm_D = 0;   // (a view, not owned)
    DevBuf<unsigned char> d_hmulti;      // problem tables and work areas of the *_multi calls
    DevBuf<int32_t> d_horder;
    DevBuf<double> d_hwork;              // L, alpha, beta, gamma (T x 2 each), mind / dist (2T)
    DevBuf<int32_t> d_hlab;              // labels (two generations), states: 3T
    DevBuf<uint8_t> d_hbt;               // Viterbi back-pointer maps
    DevBuf<double> d_hpart;              // column-pass partials
    DevBuf<double> d_hsmall;             // params (12 D + scalars), sums (4 D), centers (2 D), scalars
    DevBuf<double> d_hhist;              // logprob of every EM iteration
    DevBuf<int> d_hst;                   // k-means counters
    // Louvain tail (k_louvain.hip): the graph A (lv_m x lv_m) and its _Status vectors: diag, row sums, gdegrees (m each),
    // A.sum()'s chunk sums, diag.sum(), total_weight
    DevBuf<double> d_lvA; int64_t lv_m = 0;
    DevBuf<double> d_lvvec;
    DevBuf<int32_t> d_lvrows;
    DevBuf<unsigned char> d_lvwork;      // per-call inputs, outputs and scratch
    // a map being counted from read pairs (k_buildmap.hip), between hicmi_map_begin and hicmi_map_finish: the m x m
    // 64-bit counts (map_cells non-null: a build is open; the finish converts them in place into the doubles of the
    // matrix), first_bin on the device, and the staging of a chunk of pairs
    DevBuf<double> map_cells; int64_t map_m = 0, map_res = 0, map_pairs = 0;
    DevBuf<int32_t> d_map_first;
    std::vector<int32_t> map_first; std::vector<int64_t> map_size;
    DevBuf<unsigned char> d_map_chunk;
    // a lifted build (hicmi_map_begin_lifted) keeps its lift tables on the device as well (map_lift.seq !=
    // nullptr): map_first then describes the assembled sequences, map_size still the scaffolds; map_lift_seq is the host's
    // copy of the sequence of every scaffold.  d_stat_*: the tables and counters of a hicmi_pair_stats call
    DevBuf<unsigned char> d_map_lift; LiftTables map_lift; std::vector<int32_t> map_lift_seq;
    DevBuf<unsigned char> d_stat_lift;
    DevBuf<unsigned long long> d_stat_out;
    // spanning depth (k_spans.hip), between hicmi_span_begin and hicmi_span_finish (span_marks non-null: a
    // build is open): the marks of n_cells cells with the five counters behind them, the lift tables and cell_first on the
    // device, and the host's copies a chunk of pairs and the records of a finish are checked against
    DevBuf<unsigned long long> span_marks;
    DevBuf<unsigned char> d_span_lift; LiftTables span_lift; SpanGrid span_grid;
    DevBuf<int64_t> d_span_first;
    std::vector<int64_t> span_size, span_seq_first;
    int64_t span_pairs = 0;
    // end support (k_ends.hip), between hicmi_ends_begin and hicmi_ends_finish (ends_table non-null: a build
    // is open): the table of ends_cells counters with the six kinds behind them, the lift tables and the ranks on the
    // device, and the host's copy of the sizes a chunk of pairs is checked against
    DevBuf<unsigned long long> ends_table; int64_t ends_cells = 0;
    DevBuf<unsigned char> d_ends_lift; LiftTables ends_lift; EndsGrid ends_grid;
    DevBuf<int32_t> d_ends_rank;
    std::vector<int64_t> ends_size;
    // anchoring (k_anchor.hip), between hicmi_anchor_begin and hicmi_anchor_finish (anchor_table non-null: a
    // build is open): the table of anchor_cells counters with the six kinds behind them, the lift tables and the blocks
    // ([first n_scaf][seq_first n_seq + 1]; in rank mode target and rank, n_scaf each) on the device, and the host's copy
    // of the sizes a chunk of pairs is checked against
    DevBuf<unsigned long long> anchor_table; int64_t anchor_cells = 0;
    DevBuf<unsigned char> d_anchor_lift; LiftTables anchor_lift; AnchorGrid anchor_grid;
    DevBuf<int64_t> d_anchor_first;
    DevBuf<int32_t> d_anchor_target;
    std::vector<int64_t> anchor_size;
    // seat support (k_seats.hip), inside one hicmi_seats_resident call: the table of the blocks of all placed
    // scaffolds with the five kinds behind it, the lift tables, the blocks ([first n_scaf][seq_first n_seq + 1]) and the
    // ranks on the device; all four are released before the call returns
    DevBuf<unsigned long long> seats_table;
    DevBuf<unsigned char> d_seats_lift;
    DevBuf<int64_t> d_seats_first;
    DevBuf<int32_t> d_seats_rank;
    // the end-link graph (k_links.hip), between hicmi_links_resident and hicmi_pairs_drop: the find-or-insert
    // table ([keys cap][counts cap][LINKS_EXTRAS]), the compacted (key, count) records ([keys][counts]) and the scaffold
    // sizes on the device, and the rows of the last call on the host, sorted by (lo, hi); links_ready: there are rows to fetch
    DevBuf<unsigned long long> d_links_table, d_links_recs;
    DevBuf<int64_t> d_links_size;
    // hicmi_links_lifted, for the time of one call: the lift tables as lift_upload lays them out, the sequence sizes
    DevBuf<unsigned char> d_links_lift;
    DevBuf<int64_t> d_links_seq_size;
    std::vector<int32_t> links_lo, links_hi;
    std::vector<uint64_t> links_counts;
    bool links_ready = false;
    int64_t links_records = 0, links_slots = 0;       // of the last call: used slots, slots of its table
    double links_sort_ms = 0.0;                       // and the host's sort of the records, in milliseconds
    // the resident pair store (k_pairs.hip), between hicmi_pairs_begin / hicmi_pairs_file and hicmi_pairs_drop
    // (d_pairs_intra non-null: the context has a store): the kept pairs in four arrays of one capacity, pairs_len of
    // them in use, intra[n_scaf] with the device's copy of the length behind it, the offsets of a chunk's workgroups,
    // pinned memory the length comes back into, and the host's copy of the sizes
    DevBuf<int32_t> d_pairs_scaf_a, d_pairs_scaf_b;
    DevBuf<int64_t> d_pairs_pos_a, d_pairs_pos_b;
    DevBuf<unsigned long long> d_pairs_intra;
    DevBuf<long long> d_pairs_work;
    PinBuf<unsigned long long> pin_pairs_len;
    int64_t pairs_len = 0;
    std::vector<int64_t> pairs_size;
    // plot support
    DevBuf<int32_t> d_plot_order;
    DevBuf<unsigned char> d_plot_work;
    DevBuf<double> d_plot_img;
    // pinned staging: pageable hipMemcpyAsync takes a slow, serialising path in the runtime, which hurts when
    // several contexts are driven from different host threads
    PinBuf<char> pin_up; size_t pin_up_off = 0;
    PinBuf<char> pin_down;

    // timing
    int timing = 0;                                       // 0 off, 1 every family, 2 only the families launched a few times per map
    double ms[F_COUNT] = {0}; int64_t launches[F_COUNT] = {0}; double bytes[F_COUNT] = {0};
    // nn-chain counters since the last hicmi_timing_reset (reported by hicmi_nnchain_stats)
    double nn_scans = 0, nn_scan_cols = 0, nn_cache_hits = 0, nn_merges = 0; int64_t nn_retries = 0;
};

namespace {
hipError_t sync_stream(hicmi_ctx* c);

struct Timed {
    hicmi_ctx* c; int fam; hipEvent_t a = nullptr, b = nullptr; hipStream_t st;
    Timed(hicmi_ctx* ctx, int f, double algo_bytes, hipStream_t on_stream = nullptr) : c(ctx), fam(f), st(on_stream ? on_stream : ctx->stream)
    {
        c->launches[f]++; c->bytes[f] += algo_bytes;
        if (!on()) return;
        a = grab(); b = grab();
        hipEventRecord(a, st);
    }
    // Event pairs around the hundreds of small launches of the scans and of Part 2 cost about 10 ms per 16k map;
    // mode 2 keeps them for the families that are launched a handful of times (the dominant kernel is one of them).
    bool on() const { return c->timing == 1 || (c->timing == 2 && (fam <= F_RANK_INVERT || fam >= F_PRESORT)); }
    ~Timed()
    {
        if (!on()) return;
        hipEventRecord(b, st);
        c->tev.regions.push_back({fam, a, b});
    }
    hipEvent_t grab()
    {
        if (!c->tev.pool.empty()) { hipEvent_t e = c->tev.pool.back(); c->tev.pool.pop_back(); return e; }
        hipEvent_t e; hipEventCreate(&e); return e;
    }
};

int resolve_timing(hicmi_ctx* c)
{
    if (c->tev.regions.empty()) return HICMI_OK;
    HIPCHK(sync_stream(c));
    if (c->stream2) HIPCHK(hipStreamSynchronize(c->stream2));
    // a region whose elapsed time cannot be read is an error, not a smaller sum (the events go back to the pool either way)
    int dropped = 0, dropped_fam = 0;
    hipError_t dropped_err = hipSuccess;
    for (auto& r : c->tev.regions) {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, r.a, r.b);
        if (e == hipSuccess) c->ms[r.fam] += ms;
        else if (dropped++ == 0) { dropped_fam = r.fam; dropped_err = e; }
        c->tev.pool.push_back(r.a); c->tev.pool.push_back(r.b);
    }
    c->tev.regions.clear();
    if (dropped)
        return fail(HICMI_EHIP, "hipEventElapsedTime failed for %d timed region(s), the first of family %s: %s", dropped,
                    kFamilyNames[dropped_fam], hipGetErrorString(dropped_err));
    return HICMI_OK;
}


hipError_t sync_stream(hicmi_ctx* c)
{
    hipError_t e = hipStreamSynchronize(c->stream);
    c->pin_up_off = 0;                                   // everything staged for upload has been consumed
    return e;
}

// copy `bytes` from pageable host memory to the device through the pinned upload arena (asynchronous)
int upload(hicmi_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return HICMI_OK;
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (c->pin_up_off + need > (size_t)c->pin_up.capacity()) {
        HIPCHK(sync_stream(c));
        if (need > (size_t)c->pin_up.capacity()) HIPCHK(c->pin_up.reserve((int64_t)std::max<size_t>(need * 2, (size_t)1 << 20)));
    }
    char* slot = c->pin_up + c->pin_up_off;
    memcpy(slot, src, bytes);
    c->pin_up_off += need;
    HIPCHK(hipMemcpyAsync(dst, slot, bytes, hipMemcpyHostToDevice, c->stream));
    return HICMI_OK;
}

int ensure_pin_down(hicmi_ctx* c, size_t bytes)
{
    if (bytes > (size_t)c->pin_down.capacity()) HIPCHK(c->pin_down.reserve((int64_t)std::max<size_t>(bytes * 2, (size_t)1 << 20)));
    return HICMI_OK;
}

// device -> pageable host through the pinned download buffer; synchronises the stream
int download(hicmi_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) { HIPCHK(sync_stream(c)); return HICMI_OK; }
    int rc_pin = ensure_pin_down(c, bytes);
    if (rc_pin) return rc_pin;
    HIPCHK(hipMemcpyAsync(c->pin_down, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_stream(c));
    memcpy(dst, c->pin_down, bytes);
    return HICMI_OK;
}

// every failed device allocation is reported alike (the literal is cut in two: no allocation call is spelt in this file)
int no_memory(size_t bytes, hipError_t e)
{
    return fail(HICMI_ENOMEM, "hipMalloc" "(%lld bytes): %s", (long long)bytes, hipGetErrorString(e));
}

// room for `need` elements in `buf` (DevBuf::reserve: grows only, never copies)
template <typename T>
int ensure(DevBuf<T>& buf, int64_t need)
{
    const hipError_t e = buf.reserve(need);
    return e == hipSuccess ? HICMI_OK : no_memory(DevBuf<T>::bytes_for(need), e);
}

// ensure_all(a, need_a, b, need_b, ...): the whole group holds its memory, or none of it does (reserve_all)
template <typename... Args>
int ensure_all(Args&&... args)
{
    size_t failed_bytes = 0;
    const hipError_t e = reserve_all(&failed_bytes, args...);
    return e == hipSuccess ? HICMI_OK : no_memory(failed_bytes, e);
}

// a switch of the environment as its caller read it: "1" on, "0" off, anything else (unset too) the caller's default
bool plain_switch(const char* value, bool dflt)
{
    if (value && !strcmp(value, "1")) return true;
    if (value && !strcmp(value, "0")) return false;
    return dflt;
}

// an integer setting `name` of the environment as its caller read it, within 1 .. 2^log2_most; unset: `dflt`
int setting_in_range(const char* name, const char* value, int log2_most, int64_t dflt, int64_t* out)
{
    *out = dflt;
    if (value) {
        const long long v = atoll(value);
        if (v < 1 || v > ((long long)1 << log2_most)) return fail(HICMI_EINVAL, "%s = %s outside 1 .. 2^%d", name, value, log2_most);
        *out = v;
    }
    return HICMI_OK;
}

// the counters of a build that opens, zeroed, and the tables uploaded before them off the upload arena
int zero_and_wait(hicmi_ctx* c, void* counters, size_t bytes)
{
    hipError_t e = hipMemsetAsync(counters, 0, bytes, c->stream);
    if (e != hipSuccess) return fail(HICMI_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e));
    if ((e = sync_stream(c)) != hipSuccess) return fail(HICMI_EHIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    return HICMI_OK;
}

// after a launch on the context's stream: the launch's error or the stream's, reported as "<doing>: <the error>"
int wait_launched(hicmi_ctx* c, const char* doing)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = sync_stream(c);
    return e == hipSuccess ? HICMI_OK : fail(HICMI_EHIP, "%s: %s", doing, hipGetErrorString(e));
}

// a table of m counters with n_kinds more behind it: the kinds come down first, then the table straight into table_out,
// and kinds_out is written only when the table is down
int download_table(hicmi_ctx* c, const unsigned long long* table, int64_t m, int n_kinds, uint64_t* table_out, uint64_t* kinds_out)
{
    std::vector<uint64_t> kinds((size_t)n_kinds);
    int rc = download(c, kinds.data(), table + m, sizeof(uint64_t) * kinds.size());
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(table_out, table, sizeof(uint64_t) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_stream(c));
    memcpy(kinds_out, kinds.data(), sizeof(uint64_t) * kinds.size());
    return HICMI_OK;
}

// a candidate's bin order is staged in LDS as int32, 160 KiB at the most
int check_candidate_bins(int64_t n_bins)
{
    if (n_bins * (int64_t)sizeof(int32_t) > 160 * 1024) return fail(HICMI_EUNSUPPORTED, "candidate longer than 40960 bins");
    return HICMI_OK;
}

// Everything derived from the matrix is gone (include/hicmi.h, "What a new matrix invalidates"): the computed sums, the
// merges, the rank matrix and its pre-sort, the cut scan's cached row, and all of Part 2 from the selection down (layout,
// arrangement, its literal score, the exact-score cache).  The snapshots (HMM slots, the Louvain graph, the window
// tables, the pair store, open builds) are copies and stay.
int forget_matrix_derived(hicmi_ctx* c)
{
    hipError_t e = hipSuccess;
    if (c->presort_n && c->stream2) e = hipStreamSynchronize(c->stream2);     // the pre-sort reads the matrix being replaced
    c->presort_n = 0;
    c->have_sums = false; c->have_rank = false; c->cached_start = -1;
    c->zraw.clear();
    c->n2 = 0; c->n_scaf = 0; c->n_arr = 0; c->h_arr_id.clear();
    c->cur_lit_version = ~0ull;
    c->cache_valid = false; c->exact_cache.clear();
    HIPCHK(e);
    return HICMI_OK;
}

void drop_matrix_state(hicmi_ctx* c)
{
    (void)forget_matrix_derived(c);
    c->c_own.reset();
    c->dC = nullptr; c->own_c = false; c->n = 0; c->ldc = 0;
    c->d_np.reset(); c->d_seq.reset();
}

int alloc_sums(hicmi_ctx* c)
{
    return ensure_all(c->d_np, c->n, c->d_seq, c->n);
}

int compute_sums(hicmi_ctx* c)
{
    if (c->have_sums) return HICMI_OK;
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    {
        Timed t(c, F_ROW_SUMS, 2.0 * 8.0 * (double)c->n * (double)c->n);
        launch_row_sums(c->dC, c->ldc, (int)c->n, c->d_np, c->d_seq, 0, 1, c->stream);
    }
    HIPCHK(hipGetLastError());
    c->have_sums = true;
    return HICMI_OK;
}

// `made` (n x n, built on the device) replaces the context's matrix state; its sums are computed
int own_matrix(hicmi_ctx* c, DevBuf<double>&& made, int64_t n)
{
    drop_matrix_state(c);
    c->c_own = std::move(made);
    c->dC = c->c_own; c->own_c = true; c->n = n; c->ldc = n;
    int rc = alloc_sums(c);
    return rc ? rc : compute_sums(c);
}

// job j of a multi-chromosome call: a context of its own, on the first job's device
int check_job_context(hicmi_ctx* const* ctxs, int64_t j)
{
    if (!ctxs[j] || !ctxs[0] || ctxs[j]->device != ctxs[0]->device) return fail(HICMI_EINVAL, "contexts must share one device");
    for (int64_t q = 0; q < j; q++) if (ctxs[q] == ctxs[j]) return fail(HICMI_EINVAL, "one context per chromosome");
    return HICMI_OK;
}
}  // namespace

extern "C" {

int hicmi_abi_version(void) { return HICMI_ABI_VERSION; }
const char* hicmi_last_error(void) { return g_err.c_str(); }

int hicmi_device_count(int* count)
{
    if (!count) return fail(HICMI_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; return fail(HICMI_EHIP, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return HICMI_OK;
}

int hicmi_create(int device, hicmi_ctx** out)
{
    if (!out) return fail(HICMI_EINVAL, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(HICMI_EHIP, "no HIP device available (%s): libhicmi has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= n) return fail(HICMI_EINVAL, "device %d out of range (0..%d)", device, n - 1);
    HIPCHK(hipSetDevice(device));
    hicmi_ctx* c = new hicmi_ctx();
    c->device = device;
    hipError_t se = hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking);
    if (se != hipSuccess) { delete c; return fail(HICMI_EHIP, "hipStreamCreate: %s", hipGetErrorString(se)); }
    c->probed_xcc = nnchain_probe_xcc(c->stream);
    // "off": every window downloads its deltas; a number n >= 1: windows of at least n scaffolds use the device short list
    if (const char* dd = getenv("HICMI_P2_DEVICE_DECIDE")) {
        if (!strcmp(dd, "off")) c->near_min_k = INT_MAX;
        else if (atoi(dd) >= 1) c->near_min_k = atoi(dd);
    }
    *out = c;
    return HICMI_OK;
}

int hicmi_destroy(hicmi_ctx* c)
{
    if (!c) return HICMI_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    delete c;
    return HICMI_OK;
}

int hicmi_stream(hicmi_ctx* c, void** stream_out)
{
    if (!c || !stream_out) return fail(HICMI_EINVAL, "NULL argument");
    *stream_out = (void*)c->stream;
    return HICMI_OK;
}

int hicmi_synchronize(hicmi_ctx* c)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

// ---------------------------------------------------------------------------------------------------
int hicmi_set_contacts_host(hicmi_ctx* c, const double* contacts, int64_t n)
{
    if (!c || !contacts || n < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (n > 65536) return fail(HICMI_EUNSUPPORTED, "n = %lld > 65536 bins: rank matrix is uint16 in this version", (long long)n);
    HIPCHK(hipSetDevice(c->device));
    drop_matrix_state(c);
    int rc = ensure(c->c_own, n * n);
    if (rc) return rc;
    c->n = n; c->ldc = n; c->dC = c->c_own; c->own_c = true;
    HIPCHK(hipMemcpyAsync(c->dC, contacts, sizeof(double) * (size_t)n * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(sync_stream(c));
    return alloc_sums(c);
}

int hicmi_set_contacts_host_f32(hicmi_ctx* c, const float* contacts, int64_t n)
{
    // BASELINE configs[4]: a 64,000-bin map stored as fp32 (16.4 GB instead of 32.8 GB on the host and over PCIe).
    // The values are widened on the device; every stage computes in fp64 on exactly those widened values.
    if (!c || !contacts || n < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (n > 65536) return fail(HICMI_EUNSUPPORTED, "n = %lld > 65536 bins: rank matrix is uint16 in this version", (long long)n);
    HIPCHK(hipSetDevice(c->device));
    drop_matrix_state(c);
    const size_t cells = (size_t)n * (size_t)n;
    int rc = ensure(c->c_own, n * n);
    if (rc) return rc;
    c->n = n; c->ldc = n; c->dC = c->c_own; c->own_c = true;
    // the fp32 image is staged in the tail of the fp64 buffer and widened back to front, row block by row block
    float* d_stage = reinterpret_cast<float*>(c->dC) + cells;
    HIPCHK(hipMemcpyAsync(d_stage, contacts, sizeof(float) * cells, hipMemcpyHostToDevice, c->stream));
    launch_widen_f32(d_stage, c->dC, (int64_t)cells, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_stream(c));
    return alloc_sums(c);
}

int hicmi_set_contacts_device(hicmi_ctx* c, const double* d_contacts, int64_t n, int64_t ld)
{
    if (!c || !d_contacts || n < 1 || ld < n) return fail(HICMI_EINVAL, "bad arguments");
    if (n > 65536) return fail(HICMI_EUNSUPPORTED, "n = %lld > 65536 bins: rank matrix is uint16 in this version", (long long)n);
    HIPCHK(hipSetDevice(c->device));
    drop_matrix_state(c);
    c->n = n; c->ldc = ld; c->dC = const_cast<double*>(d_contacts); c->own_c = false;
    return alloc_sums(c);
}

int hicmi_contacts_device(hicmi_ctx* c, void** d_contacts_out, int64_t* n_out, int64_t* ld_out)
{
    if (!c || !d_contacts_out || !n_out || !ld_out) return fail(HICMI_EINVAL, "NULL argument");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    *d_contacts_out = (void*)c->dC; *n_out = c->n; *ld_out = c->ldc;
    return HICMI_OK;
}

int hicmi_set_row_shard(hicmi_ctx* c, int64_t first, int64_t stride)
{
    if (!c || stride < 1 || first < 0 || first >= stride) return fail(HICMI_EINVAL, "row shard needs 0 <= first < stride");
    c->shard_first = first; c->shard_stride = stride;
    c->have_rank = false; c->cached_start = -1;
    if (c->presort_n && c->stream2) (void)hipStreamSynchronize(c->stream2);
    c->presort_n = 0;
    return HICMI_OK;
}

int hicmi_set_row_sums(hicmi_ctx* c, const double* np_sum, const double* seq_sum)
{
    if (!c || !np_sum || !seq_sum) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    HIPCHK(hipSetDevice(c->device));
    int rc = upload(c, c->d_np, np_sum, sizeof(double) * (size_t)c->n);
    if (rc) return rc;
    rc = upload(c, c->d_seq, seq_sum, sizeof(double) * (size_t)c->n);
    if (rc) return rc;
    HIPCHK(sync_stream(c));
    if (c->presort_n && c->stream2) HIPCHK(hipStreamSynchronize(c->stream2));
    c->presort_n = 0;                                      // the similarity keys depend on the sums,
    c->have_rank = false; c->cached_start = -1;            // and so do the rank matrix and the scan row counted from it,
    c->zraw.clear();                                       // and the merges (the distances divide by np_sum)
    c->have_sums = true;
    return HICMI_OK;
}

int hicmi_row_sums(hicmi_ctx* c, double* np_sum, double* seq_sum)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    HIPCHK(hipSetDevice(c->device));
    int rc = HICMI_OK;
    if (c->shard_stride > 1 && !c->have_sums) {
        // this shard's rows only (the other entries read 0); the caller gathers the shards and hands the complete
        // vectors back with hicmi_set_row_sums
        if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
        HIPCHK(hipMemsetAsync(c->d_np, 0, sizeof(double) * (size_t)c->n, c->stream));
        HIPCHK(hipMemsetAsync(c->d_seq, 0, sizeof(double) * (size_t)c->n, c->stream));
        {
            Timed t(c, F_ROW_SUMS, 2.0 * 8.0 * (double)c->n * (double)c->n / (double)c->shard_stride);
            launch_row_sums(c->dC, c->ldc, (int)c->n, c->d_np, c->d_seq, (int)c->shard_first, (int)c->shard_stride, c->stream);
        }
        HIPCHK(hipGetLastError());
    }
    else rc = compute_sums(c);
    if (rc) return rc;
    if (np_sum) { rc = download(c, np_sum, c->d_np, sizeof(double) * (size_t)c->n); if (rc) return rc; }
    if (seq_sum) { rc = download(c, seq_sum, c->d_seq, sizeof(double) * (size_t)c->n); if (rc) return rc; }
    if (!np_sum && !seq_sum) HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_compact(hicmi_ctx* c, const int32_t* keep, int64_t n_keep)
{
    if (!c || !keep || n_keep < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    if (n_keep > c->n) return fail(HICMI_EINVAL, "n_keep > n");
    for (int64_t i = 0; i < n_keep; i++)
        if (keep[i] < 0 || keep[i] >= c->n || (i && keep[i] <= keep[i - 1])) return fail(HICMI_EINVAL, "keep must be ascending indices in [0, n)");
    HIPCHK(hipSetDevice(c->device));
    DevBuf<int32_t> d_keep; DevBuf<double> d_new;
    int rc = ensure_all(d_keep, n_keep, d_new, n_keep * n_keep);
    if (!rc) rc = upload(c, d_keep, keep, sizeof(int32_t) * (size_t)n_keep);
    if (rc) return rc;
    launch_compact(c->dC, c->ldc, d_keep, (int)n_keep, d_new, n_keep, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_stream(c));
    d_keep.reset();
    return own_matrix(c, std::move(d_new), n_keep);
}

// A coarser map from the resident raw one: HiC-Pro's build_matrix re-run at k times the bin size.  Like
// hicmi_compact, the result replaces the context's matrix state and an adopted source is only read.
int hicmi_rebin(hicmi_ctx* c, const int32_t* group_start, int64_t m)
{
    if (!c || !group_start) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    const int64_t n = c->n;
    if (m < 1 || m > n) return fail(HICMI_EINVAL, "m = %lld outside 1 .. n = %lld", (long long)m, (long long)n);
    if (group_start[0] != 0 || group_start[m] != n)
        return fail(HICMI_EINVAL, "group_start must run from 0 to n = %lld", (long long)n);
    for (int64_t i = 0; i < m; i++)
        if (group_start[i + 1] <= group_start[i]) return fail(HICMI_EINVAL, "group_start must be strictly ascending");
    for (int64_t i = 0; i < m; i++)
        if (group_start[i + 1] - group_start[i] > REBIN_MAX_WIDTH)
            return fail(HICMI_EUNSUPPORTED, "coarse bin %lld has %d fine bins: at most %d", (long long)i,
                        group_start[i + 1] - group_start[i], REBIN_MAX_WIDTH);
    const bool plain = plain_switch(getenv("HICMI_REBIN_PLAIN"), false);
    // one image of both lists: group_start, then chunk_first
    const int64_t n_chunks = (n + REBIN_CHUNK - 1) / REBIN_CHUNK;
    std::vector<int32_t> img((size_t)(m + 1 + n_chunks + 1));
    memcpy(img.data(), group_start, sizeof(int32_t) * (size_t)(m + 1));
    {
        int64_t J = 0;
        for (int64_t ch = 0; ch <= n_chunks; ch++) {
            while (J < m && group_start[J + 1] <= ch * REBIN_CHUNK) J++;
            img[(size_t)(m + 1 + ch)] = (int32_t)J;
        }
    }
    HIPCHK(hipSetDevice(c->device));
    DevBuf<int32_t> d_lists; DevBuf<double> d_new;
    int rc = ensure_all(d_lists, (int64_t)img.size(), d_new, m * m);
    if (!rc) rc = upload(c, d_lists, img.data(), sizeof(int32_t) * img.size());
    if (rc) return rc;
    launch_rebin(c->dC, c->ldc, (int)n, d_lists, d_lists + m + 1, (int)m, d_new, plain, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_stream(c));
    d_lists.reset();
    return own_matrix(c, std::move(d_new), m);
}

// ---- a raw map counted from read pairs: HiC-Pro's build_matrix at any bin size --------------------------
// Between hicmi_map_begin and hicmi_map_finish the counts live in scratch of their own (map_cells); the context's matrix
// state is replaced only by a finish that succeeded.
static void map_abandon(hicmi_ctx* c)
{
    c->map_cells.reset(); c->d_map_first.reset(); c->d_map_lift.reset();
    c->map_lift = LiftTables();
    c->map_m = 0; c->map_res = 0; c->map_pairs = 0;
    c->map_first.clear(); c->map_size.clear(); c->map_lift_seq.clear();
}

// HICMI_BUILDMAP_PLAIN: "1" one atomic add per pair, "0" the combining kernel, anything else the default - the plain
// kernel: on the 16,000-bin bench map the combining kernel did not beat it
constexpr bool kBuildmapPlainByDefault = true;
static bool buildmap_plain()
{
    return plain_switch(getenv("HICMI_BUILDMAP_PLAIN"), kBuildmapPlainByDefault);
}

// HICMI_LIFTMAP_PLAIN: the same choice for a lifted build, read per call
constexpr bool kLiftmapPlainByDefault = true;
static bool liftmap_plain()
{
    return plain_switch(getenv("HICMI_LIFTMAP_PLAIN"), kLiftmapPlainByDefault);
}

// the lift of a build as the caller hands it over: host arrays, one entry per scaffold, and the sequences' sizes
struct LiftHost { const int32_t* seq; const int64_t* off; const uint8_t* rev; const int64_t* seq_size; int64_t n_seq; };

static int lift_check(const int64_t* scaf_size, int64_t n_scaf, const LiftHost& lift)
{
    if (!lift.seq || !lift.off || !lift.rev || !lift.seq_size || lift.n_seq < 1 || lift.n_seq > INT_MAX / 4)
        return fail(HICMI_EINVAL, "bad arguments");
    char msg[256];
    if (lift_check_tables(scaf_size, n_scaf, lift.seq, lift.off, lift.rev, lift.seq_size, lift.n_seq, msg, sizeof(msg)))
        return fail(HICMI_EINVAL, "%s", msg);
    return HICMI_OK;
}

// the lift tables as one device image of 21 bytes per scaffold, 8-byte fields first: [off][scaf_size][seq][rev]
static int lift_upload(hicmi_ctx* c, unsigned char* image, const int64_t* scaf_size, int64_t n_scaf, const LiftHost& lift,
                       LiftTables* out)
{
    int64_t* d_off = reinterpret_cast<int64_t*>(image);
    int64_t* d_size = d_off + n_scaf;
    int32_t* d_seq = reinterpret_cast<int32_t*>(d_size + n_scaf);
    uint8_t* d_rev = reinterpret_cast<uint8_t*>(d_seq + n_scaf);
    int rc = upload(c, d_off, lift.off, sizeof(int64_t) * (size_t)n_scaf);
    if (!rc) rc = upload(c, d_size, scaf_size, sizeof(int64_t) * (size_t)n_scaf);
    if (!rc) rc = upload(c, d_seq, lift.seq, sizeof(int32_t) * (size_t)n_scaf);
    if (!rc) rc = upload(c, d_rev, lift.rev, (size_t)n_scaf);
    if (rc) return rc;
    out->off = d_off; out->scaf_size = d_size; out->seq = d_seq; out->rev = d_rev;
    out->n_scaf = (int32_t)n_scaf; out->n_seq = (int32_t)lift.n_seq;
    return HICMI_OK;
}

// hicmi_map_begin and, with a lift, hicmi_map_begin_lifted: the grid is cut from the scaffolds or from the sequences
static int map_open(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, int64_t resolution, const LiftHost* lift)
{
    if (!c || !scaf_size || n_scaf < 1 || n_scaf > INT_MAX / 2) return fail(HICMI_EINVAL, "bad arguments");
    if (resolution < 1) return fail(HICMI_EINVAL, "resolution %lld is below 1", (long long)resolution);
    if (lift) { int rc = lift_check(scaf_size, n_scaf, *lift); if (rc) return rc; }
    const int64_t* grid = lift ? lift->seq_size : scaf_size;
    const int64_t n_grid = lift ? lift->n_seq : n_scaf;
    const char* what = lift ? "sequence" : "scaffold";
    std::vector<int32_t> first((size_t)n_grid);
    int64_t m = 0;
    for (int64_t s = 0; s < n_grid; s++) {
        if (grid[s] < 0) return fail(HICMI_EINVAL, "%s %lld has the negative size %lld", what, (long long)s, (long long)grid[s]);
        first[(size_t)s] = (int32_t)m;
        m += grid[s] / resolution + (grid[s] % resolution != 0);
        if (m > 65536)
            return fail(HICMI_EUNSUPPORTED, "resolution %lld needs more than 65536 bins: rank matrix is uint16 in this version",
                        (long long)resolution);
    }
    if (m < 1) return fail(HICMI_EINVAL, "the %ss have no bins", what);
    HIPCHK(hipSetDevice(c->device));
    map_abandon(c);                                           // a begin without a finish is given up
    static_assert(sizeof(uint64_t) == sizeof(double), "the counts are converted in place");
    int rc = lift ? ensure_all(c->map_cells, m * m, c->d_map_first, n_grid, c->d_map_lift, 21 * n_scaf)
                  : ensure_all(c->map_cells, m * m, c->d_map_first, n_grid);
    if (rc) return rc;
    rc = upload(c, c->d_map_first, first.data(), sizeof(int32_t) * (size_t)n_grid);
    if (!rc && lift) rc = lift_upload(c, c->d_map_lift, scaf_size, n_scaf, *lift, &c->map_lift);
    if (!rc) rc = zero_and_wait(c, c->map_cells, sizeof(uint64_t) * (size_t)m * (size_t)m);
    if (rc) { map_abandon(c); return rc; }
    c->map_m = m; c->map_res = resolution; c->map_pairs = 0;
    c->map_first = std::move(first);
    c->map_size.assign(scaf_size, scaf_size + n_scaf);
    if (lift) c->map_lift_seq.assign(lift->seq, lift->seq + n_scaf);
    return HICMI_OK;
}

int hicmi_map_begin(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, int64_t resolution)
{
    return map_open(c, scaf_size, n_scaf, resolution, nullptr);
}

int hicmi_map_begin_lifted(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                           const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, int64_t resolution)
{
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    return map_open(c, scaf_size, n_scaf, resolution, &lift);
}

// the four arrays of a chunk, one after the other in one device buffer (8-byte fields first)
struct MapChunk { int64_t *pos_a, *pos_b; int32_t *scaf_a, *scaf_b; };
static MapChunk map_chunk_at(unsigned char* base, int64_t n)
{
    MapChunk k;
    k.pos_a = reinterpret_cast<int64_t*>(base);
    k.pos_b = k.pos_a + n;
    k.scaf_a = reinterpret_cast<int32_t*>(k.pos_b + n);
    k.scaf_b = k.scaf_a + n;
    return k;
}

// every scaffold index and position of a chunk against the scaffold sizes; with lift_seq, also the pairs that have an end
// on a dropped scaffold
static int check_pairs(const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, int64_t* unlifted_out)
{
    int64_t unlifted = 0;
    for (int64_t p = 0; p < n; p++) {
        if (scaf_a[p] < 0 || scaf_a[p] >= n_scaf || scaf_b[p] < 0 || scaf_b[p] >= n_scaf)
            return fail(HICMI_EINVAL, "pair %lld names a scaffold outside 0 .. %lld", (long long)p, (long long)(n_scaf - 1));
        if (pos_a[p] < 1 || pos_a[p] > scaf_size[scaf_a[p]] || pos_b[p] < 1 || pos_b[p] > scaf_size[scaf_b[p]])
            return fail(HICMI_EINVAL, "pair %lld has a position outside 1 .. the size of its scaffold", (long long)p);
        if (lift_seq) unlifted += lift_seq[scaf_a[p]] < 0 || lift_seq[scaf_b[p]] < 0;
    }
    if (unlifted_out) *unlifted_out = unlifted;
    return HICMI_OK;
}

// a chunk of host arrays on its way into the context's staging (d_map_chunk, which holds nothing between calls)
static int stage_chunk(hicmi_ctx* c, const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                       MapChunk* out)
{
    int rc = ensure(c->d_map_chunk, 24 * n);
    if (rc) return rc;
    const MapChunk k = *out = map_chunk_at(c->d_map_chunk, n);
    rc = upload(c, k.pos_a, pos_a, sizeof(int64_t) * (size_t)n);
    if (!rc) rc = upload(c, k.pos_b, pos_b, sizeof(int64_t) * (size_t)n);
    if (!rc) rc = upload(c, k.scaf_a, scaf_a, sizeof(int32_t) * (size_t)n);
    if (!rc) rc = upload(c, k.scaf_b, scaf_b, sizeof(int32_t) * (size_t)n);
    return rc;
}

// the counters of k_pair_stats, [decay 256][cis n_seq][trans n_seq][unlifted], added to the caller's arrays
static void stats_add(const uint64_t* got, int64_t n_seq, uint64_t* decay_out, uint64_t* seq_cis_out, uint64_t* seq_trans_out,
                      uint64_t* unlifted_out)
{
    for (int k = 0; k < LIFT_DECAY_SLOTS; k++) decay_out[k] += got[k];
    for (int64_t q = 0; q < n_seq; q++) {
        seq_cis_out[q] += got[LIFT_DECAY_SLOTS + q];
        seq_trans_out[q] += got[LIFT_DECAY_SLOTS + n_seq + q];
    }
    *unlifted_out += got[LIFT_DECAY_SLOTS + 2 * n_seq];
}

int hicmi_map_add_pairs(hicmi_ctx* c, const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b,
                        int64_t n)
{
    if (!c || n < 0 || (n > 0 && (!scaf_a || !pos_a || !scaf_b || !pos_b))) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->map_cells) return fail(HICMI_EINVAL, "hicmi_map_add_pairs without hicmi_map_begin");
    const int64_t n_scaf = (int64_t)c->map_size.size();
    int64_t unlifted = 0;                                     // a lifted build skips the pairs with an end on a dropped scaffold
    int rc_pairs = check_pairs(scaf_a, pos_a, scaf_b, pos_b, n, c->map_size.data(), n_scaf,
                               c->map_lift.seq ? c->map_lift_seq.data() : nullptr, &unlifted);
    if (rc_pairs) return rc_pairs;
    if (n == 0) return HICMI_OK;
    HIPCHK(hipSetDevice(c->device));
    // a HIP error from here on gives the build up: what was counted so far cannot be told
    MapChunk k;
    int rc = stage_chunk(c, scaf_a, pos_a, scaf_b, pos_b, n, &k);
    if (!rc) {
        launch_buildmap_add(k.scaf_a, k.pos_a, k.scaf_b, k.pos_b, n, c->d_map_first, (int)c->map_first.size(), c->map_res,
                            (int)c->map_m, c->map_cells, c->map_lift.seq ? liftmap_plain() : buildmap_plain(), c->map_lift,
                            c->stream);
        rc = wait_launched(c, "counting a chunk of pairs");
    }
    if (rc) { map_abandon(c); return rc; }
    c->map_pairs += n - unlifted;
    return HICMI_OK;
}

// The statistics of a chunk of pairs under a lift, added to the caller's arrays.  No matrix state.
int hicmi_pair_stats(hicmi_ctx* c, const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                     const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                     const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, uint64_t* decay_out, uint64_t* seq_cis_out,
                     uint64_t* seq_trans_out, uint64_t* unlifted_out)
{
    if (!c || n < 0 || (n > 0 && (!scaf_a || !pos_a || !scaf_b || !pos_b)) || !scaf_size || n_scaf < 1 || n_scaf > INT_MAX / 2 ||
        !decay_out || !seq_cis_out || !seq_trans_out || !unlifted_out)
        return fail(HICMI_EINVAL, "bad arguments");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    int rc = lift_check(scaf_size, n_scaf, lift);
    if (!rc) rc = check_pairs(scaf_a, pos_a, scaf_b, pos_b, n, scaf_size, n_scaf, nullptr, nullptr);
    if (rc || n == 0) return rc;
    HIPCHK(hipSetDevice(c->device));
    const int64_t n_out = LIFT_DECAY_SLOTS + 2 * n_seq + 1;
    rc = ensure(c->d_stat_lift, 21 * n_scaf);
    if (!rc) rc = ensure(c->d_stat_out, n_out);
    if (rc) return rc;
    LiftTables tables;
    MapChunk k;
    rc = lift_upload(c, c->d_stat_lift, scaf_size, n_scaf, lift, &tables);
    if (!rc) rc = stage_chunk(c, scaf_a, pos_a, scaf_b, pos_b, n, &k);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->d_stat_out, 0, sizeof(uint64_t) * (size_t)n_out, c->stream));
    launch_pair_stats(k.scaf_a, k.pos_a, k.scaf_b, k.pos_b, n, tables, c->d_stat_out, c->stream);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> got((size_t)n_out);
    rc = download(c, got.data(), c->d_stat_out, sizeof(uint64_t) * (size_t)n_out);
    if (rc) return rc;
    stats_add(got.data(), n_seq, decay_out, seq_cis_out, seq_trans_out, unlifted_out);
    return HICMI_OK;
}

// the counts become the context's matrix; `on` is the stream the conversion runs on (the driver uses one for all maps)
static int map_install(hicmi_ctx* c, hipStream_t on, int64_t* pairs_out)
{
    launch_buildmap_finish(c->map_cells, (int)c->map_m, on);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(on);
    if (e != hipSuccess) { map_abandon(c); return fail(HICMI_EHIP, "converting the counts: %s", hipGetErrorString(e)); }
    DevBuf<double> made = std::move(c->map_cells);            // ownership moves to the context below
    const int64_t m = c->map_m, pairs = c->map_pairs;
    map_abandon(c);
    int rc = own_matrix(c, std::move(made), m);
    if (rc) return rc;
    if (pairs_out) *pairs_out = pairs;
    return HICMI_OK;
}

int hicmi_map_finish(hicmi_ctx* c, int64_t* pairs_out)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (!c->map_cells) return fail(HICMI_EINVAL, "hicmi_map_finish without hicmi_map_begin");
    HIPCHK(hipSetDevice(c->device));
    return map_install(c, c->stream, pairs_out);
}

// ---- scaffolds cut into pieces: the tables of a split as the caller hands them over --------------------------
struct SplitHost { const int32_t* piece_first; const int64_t* piece_start; int64_t n_piece; };

// HICMI_SPLIT_PLAIN: "1" the literal kernel (a scan over the pieces, one atomic add per counter and pair), "0" the
// combining kernel, anything else the default; read per call
constexpr bool kSplitPlainByDefault = false;
static bool split_plain()
{
    return plain_switch(getenv("HICMI_SPLIT_PLAIN"), kSplitPlainByDefault);
}

static int split_check(const int64_t* scaf_size, int64_t n_scaf, const SplitHost& split)
{
    if (!scaf_size || n_scaf < 1 || n_scaf > INT_MAX / 4 || !split.piece_first || !split.piece_start || split.n_piece < n_scaf ||
        split.n_piece > INT_MAX / 4)                              // 4 n_piece counters, each a 32-bit key of the kernel's table
        return fail(HICMI_EINVAL, "bad arguments");
    char msg[256];
    if (split_check_tables(scaf_size, n_scaf, split.piece_first, split.piece_start, split.n_piece, msg, sizeof(msg)))
        return fail(HICMI_EINVAL, "%s", msg);
    return HICMI_OK;
}

// the sizes of the pieces of tables that passed split_check: the grid a split map is cut from
static std::vector<int64_t> split_piece_sizes(const int64_t* scaf_size, int64_t n_scaf, const SplitHost& split)
{
    std::vector<int64_t> out((size_t)split.n_piece);
    for (int64_t s = 0; s < n_scaf; s++)
        for (int64_t k = split.piece_first[s]; k < split.piece_first[s + 1]; k++)
            out[(size_t)k] = (k + 1 < split.piece_first[s + 1] ? split.piece_start[k + 1] : scaf_size[s]) - split.piece_start[k];
    return out;
}

// the tables as one device image, 8-byte fields first: [piece_start n_piece][piece_first n_scaf + 1]
static int64_t split_image_bytes(int64_t n_scaf, int64_t n_piece) { return 8 * n_piece + 4 * (n_scaf + 1); }
static int split_upload(hicmi_ctx* c, unsigned char* image, int64_t n_scaf, const SplitHost& split, SplitTables* out)
{
    int64_t* d_start = reinterpret_cast<int64_t*>(image);
    int32_t* d_first = reinterpret_cast<int32_t*>(d_start + split.n_piece);
    int rc = upload(c, d_start, split.piece_start, sizeof(int64_t) * (size_t)split.n_piece);
    if (!rc) rc = upload(c, d_first, split.piece_first, sizeof(int32_t) * (size_t)(n_scaf + 1));
    if (rc) return rc;
    out->piece_start = d_start; out->piece_first = d_first;
    out->n_scaf = (int32_t)n_scaf; out->n_piece = (int32_t)split.n_piece;
    return HICMI_OK;
}

// A chunk of pairs on host arrays moved to the pieces, and what it adds to the counters of the pieces.  No matrix state,
// no open build: the chunk is staged in d_map_chunk, which holds nothing between calls, the rest in buffers of the call.
int hicmi_split_pairs(hicmi_ctx* c, const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n,
                      const int64_t* scaf_size, int64_t n_scaf, const int32_t* piece_first, const int64_t* piece_start, int64_t n_piece,
                      int32_t* piece_a_out, int64_t* pos_a_out, int32_t* piece_b_out, int64_t* pos_b_out, uint64_t* counters_out)
{
    if (!c || n < 0 || n > INT_MAX || !counters_out ||
        (n > 0 && (!scaf_a || !pos_a || !scaf_b || !pos_b || !piece_a_out || !pos_a_out || !piece_b_out || !pos_b_out)))
        return fail(HICMI_EINVAL, "bad arguments");
    const SplitHost split{piece_first, piece_start, n_piece};
    int rc = split_check(scaf_size, n_scaf, split);
    if (!rc) rc = check_pairs(scaf_a, pos_a, scaf_b, pos_b, n, scaf_size, n_scaf, nullptr, nullptr);
    if (rc || n == 0) return rc;
    HIPCHK(hipSetDevice(c->device));
    DevBuf<unsigned char> d_tables;
    DevBuf<unsigned long long> d_counters;
    const int64_t n_counters = SPLIT_COUNTERS * n_piece;
    rc = ensure_all(d_tables, split_image_bytes(n_scaf, n_piece), d_counters, n_counters);
    if (rc) return rc;
    SplitTables tables;
    MapChunk k;
    rc = split_upload(c, d_tables, n_scaf, split, &tables);
    if (!rc) rc = stage_chunk(c, scaf_a, pos_a, scaf_b, pos_b, n, &k);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d_counters, 0, sizeof(uint64_t) * (size_t)n_counters, c->stream));
    launch_split_pairs(k.scaf_a, k.pos_a, k.scaf_b, k.pos_b, n, tables, d_counters, split_plain(), c->stream);
    HIPCHK(hipGetLastError());
    // everything comes down before an output is written
    std::vector<unsigned char> moved((size_t)(24 * n));
    std::vector<uint64_t> got((size_t)n_counters);
    rc = download(c, moved.data(), c->d_map_chunk, moved.size());
    if (!rc) rc = download(c, got.data(), d_counters, sizeof(uint64_t) * got.size());
    if (rc) return rc;
    const MapChunk h = map_chunk_at(moved.data(), n);
    memcpy(pos_a_out, h.pos_a, sizeof(int64_t) * (size_t)n);
    memcpy(pos_b_out, h.pos_b, sizeof(int64_t) * (size_t)n);
    memcpy(piece_a_out, h.scaf_a, sizeof(int32_t) * (size_t)n);
    memcpy(piece_b_out, h.scaf_b, sizeof(int32_t) * (size_t)n);
    for (int64_t q = 0; q < n_counters; q++) counters_out[q] += got[(size_t)q];
    return HICMI_OK;
}

// HICMI_BUILDMAP_CHUNK_PAIRS, the pairs of one chunk of a pass over a pair file; read per call
static int chunk_pairs_setting(int64_t* out)
{
    return setting_in_range("HICMI_BUILDMAP_CHUNK_PAIRS", getenv("HICMI_BUILDMAP_CHUNK_PAIRS"), 28, (int64_t)1 << 22, out);
}

// The one loop over the chunks of a pair file, on the stream of the context c: chunk t + 1 is parsed into the other pinned
// buffer while chunk t is uploaded and handed to on_chunk(device arrays, n), which launches on that stream and returns
// nothing, or an error code that ends the pass.  stats[0 .. 3] receive the parser's sums and stats[4] the chunks, added to
// what they hold; `doing` names the work in the message of a HIP error.
extern "C++" {
template <typename OnChunk>
static int pair_file_pass(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names, const int64_t* scaf_size,
                          hicmi_ctx* c, int threads, int64_t chunk_pairs, int64_t* stats, const char* doing, OnChunk&& on_chunk)
{
    // everything the pass owns: two pinned chunks for the parser, two device chunks for the kernels
    PinBuf<unsigned char> pin[2]; DevBuf<unsigned char> dev[2];
    int64_t file_bytes = -1;
    {
        // no chunk holds more pairs than the file has room for (a line of six columns is at least 12 bytes)
        FILE* fh = fopen(path, "rb");
        if (!fh) return fail(HICMI_EINVAL, "cannot open %s", path);
        if (fseeko(fh, 0, SEEK_END) == 0) file_bytes = (int64_t)ftello(fh);
        fclose(fh);
        if (file_bytes < 0) return fail(HICMI_EINVAL, "cannot tell the size of %s", path);
        chunk_pairs = std::max<int64_t>(1, std::min(chunk_pairs, file_bytes / 12 + 1));
    }
    const size_t chunk_bytes = (size_t)chunk_pairs * 24;
    for (int b = 0; b < 2; b++) {
        HIPCHK(pin[b].reserve((int64_t)chunk_bytes));
        int rc = ensure(dev[b], (int64_t)chunk_bytes);
        if (rc) return rc;
    }
    int64_t next = 0, n_here = 0, st[4];
    auto parse = [&](int b) {
        const MapChunk h = map_chunk_at(pin[b], chunk_pairs);
        int prc = hicmi_parse_valid_pairs(path, names_blob, name_off, n_names, scaf_size, threads, next, chunk_pairs, h.scaf_a, h.pos_a,
                                          h.scaf_b, h.pos_b, &n_here, &next, st);
        if (!prc) { stats[0] += st[0]; stats[1] += st[1]; stats[2] += st[2]; stats[3] += st[3]; }
        return prc;
    };
    int cur = 0;
    int rc = parse(cur);
    if (rc) return rc;
    for (;;) {
        const int64_t n = n_here;
        if (n > 0) {
            const MapChunk h = map_chunk_at(pin[cur], chunk_pairs), d = map_chunk_at(dev[cur], chunk_pairs);
            HIPCHK(hipMemcpyAsync(d.pos_a, h.pos_a, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d.pos_b, h.pos_b, sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d.scaf_a, h.scaf_a, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(d.scaf_b, h.scaf_b, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            if constexpr (std::is_void<decltype(on_chunk(d, n))>::value) on_chunk(d, n);
            else if ((rc = on_chunk(d, n)) != HICMI_OK) {          // an on_chunk that can fail ends the pass
                (void)hipStreamSynchronize(c->stream);             // the copies out of the pinned buffers are done
                return rc;
            }
            HIPCHK(hipGetLastError());
            stats[4]++;
        }
        const bool last = next >= file_bytes;                      // the parser has taken the whole file
        if (!last) rc = parse(cur ^ 1);
        hipError_t e = hipStreamSynchronize(c->stream);            // chunk t is done: its two buffers are free again
        if (rc) return rc;
        if (e != hipSuccess) return fail(HICMI_EHIP, "%s: %s", doing, hipGetErrorString(e));
        if (last) break;
        cur ^= 1;
    }
    return HICMI_OK;
}
}  // extern "C++"

// The chunk loop of hicmi_build_maps, hicmi_lift_maps and hicmi_split_maps is pair_file_pass with the maps of every
// context counted from each chunk.  `lift` (hicmi_lift_maps): every build is a lifted one, the statistics of every chunk
// are counted beside the maps, and `stat_out` receives them when the whole file is counted.  `split` (hicmi_split_maps):
// every chunk is moved to the pieces before it is counted, the maps are cut from the pieces, and `split_out` receives the
// counters of the pieces; n_res may then be 0 (the counters alone), and ctxs[0] lends its device and its stream.
struct LiftStatsOut { uint64_t *decay, *seq_cis, *seq_trans, *unlifted; };

static int build_maps_loop(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names,
                           const int64_t* scaf_size, int64_t n_res, const int64_t* resolution, hicmi_ctx* const* ctxs, int threads,
                           int64_t* stats5, const LiftHost* lift, const LiftStatsOut* stat_out, const SplitHost* split = nullptr,
                           uint64_t* split_out = nullptr)
{
    if (!path || !names_blob || !name_off || !scaf_size || !ctxs || !stats5 || n_names < 1 || n_res < (split ? 0 : 1) ||
        (n_res > 0 && !resolution) || (split && (!split_out || !ctxs[0])))
        return fail(HICMI_EINVAL, "bad arguments");
    if (lift && (!stat_out->decay || !stat_out->seq_cis || !stat_out->seq_trans || !stat_out->unlifted))
        return fail(HICMI_EINVAL, "bad arguments");
    for (int k = 0; k < 5; k++) stats5[k] = 0;
    std::vector<int64_t> piece_size;                              // a split call: the grid of its maps
    if (split) {
        int rc = split_check(scaf_size, n_names, *split);
        if (rc) return rc;
        piece_size = split_piece_sizes(scaf_size, n_names, *split);
    }
    for (int64_t k = 0; k < n_res; k++) {
        if (!ctxs[k] || ctxs[k]->device != ctxs[0]->device) return fail(HICMI_EINVAL, "contexts must share one device");
        for (int64_t q = 0; q < k; q++) if (ctxs[q] == ctxs[k]) return fail(HICMI_EINVAL, "one context per resolution");
    }
    int64_t chunk_pairs = 0;
    int rc = chunk_pairs_setting(&chunk_pairs);
    if (rc) return rc;
    hicmi_ctx* c0 = ctxs[0];
    HIPCHK(hipSetDevice(c0->device));
    DevBuf<unsigned long long> d_stats;                          // a lifted call: the counters of k_pair_stats
    DevBuf<unsigned char> d_split; DevBuf<unsigned long long> d_split_counters;   // a split call: its tables and counters
    SplitTables split_tables;
    struct OpenBuilds {                                           // given up on every error path
        hicmi_ctx* const* ctxs; int64_t n_res; bool keep = false;
        ~OpenBuilds() { if (!keep) for (int64_t k = 0; k < n_res; k++) map_abandon(ctxs[k]); }
    } own{ctxs, n_res};
    // begin on every context first: a resolution that cannot be built is refused before the file is read
    for (int64_t k = 0; k < n_res; k++) {
        rc = split ? map_open(ctxs[k], piece_size.data(), split->n_piece, resolution[k], nullptr)
                   : map_open(ctxs[k], scaf_size, n_names, resolution[k], lift);
        if (rc) return rc;
    }
    const int64_t n_split = split ? SPLIT_COUNTERS * split->n_piece : 0;
    if (split) {
        rc = ensure_all(d_split, split_image_bytes(n_names, split->n_piece), d_split_counters, n_split);
        if (!rc) rc = split_upload(c0, d_split, n_names, *split, &split_tables);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(d_split_counters, 0, sizeof(uint64_t) * (size_t)n_split, c0->stream));
        HIPCHK(sync_stream(c0));                                  // the tables have left the upload arena
    }
    const int64_t n_stats = lift ? LIFT_DECAY_SLOTS + 2 * lift->n_seq + 1 : 0;
    if (lift) {
        rc = ensure(d_stats, n_stats);
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(uint64_t) * (size_t)n_stats, c0->stream));
    }
    const bool plain = lift ? liftmap_plain() : buildmap_plain();
    const bool literal_split = split && split_plain();
    // every chunk on c0's stream: moved to the pieces, counted on every map, its statistics counted beside them
    rc = pair_file_pass(path, names_blob, name_off, n_names, scaf_size, c0, threads, chunk_pairs, stats5, "counting a chunk of pairs",
                        [&](const MapChunk& d, int64_t n) {
                            if (split)
                                launch_split_pairs(d.scaf_a, d.pos_a, d.scaf_b, d.pos_b, n, split_tables, d_split_counters, literal_split,
                                                   c0->stream);
                            for (int64_t k = 0; k < n_res; k++) {
                                hicmi_ctx* c = ctxs[k];
                                launch_buildmap_add(d.scaf_a, d.pos_a, d.scaf_b, d.pos_b, n, c->d_map_first, (int)c->map_first.size(),
                                                    c->map_res, (int)c->map_m, c->map_cells, plain, c->map_lift, c0->stream);
                                c->map_pairs += n;
                            }
                            if (lift) launch_pair_stats(d.scaf_a, d.pos_a, d.scaf_b, d.pos_b, n, c0->map_lift, d_stats, c0->stream);
                        });
    if (rc) return rc;
    std::vector<uint64_t> got((size_t)n_stats);
    if (lift) {
        // the statistics come down before any context changes; a map has counted the pairs that were lifted
        HIPCHK(hipMemcpy(got.data(), d_stats, sizeof(uint64_t) * (size_t)n_stats, hipMemcpyDeviceToHost));
        for (int64_t k = 0; k < n_res; k++) ctxs[k]->map_pairs -= (int64_t)got[(size_t)n_stats - 1];
    }
    std::vector<uint64_t> got_split((size_t)n_split);
    if (split) HIPCHK(hipMemcpy(got_split.data(), d_split_counters, sizeof(uint64_t) * (size_t)n_split, hipMemcpyDeviceToHost));
    // every chunk is counted on every map: from here on the contexts change
    own.keep = true;
    for (int64_t k = 0; k < n_res; k++) {
        HIPCHK(hipSetDevice(ctxs[k]->device));
        rc = map_install(ctxs[k], c0->stream, nullptr);
        if (rc) { for (int64_t q = k + 1; q < n_res; q++) map_abandon(ctxs[q]); return rc; }
    }
    if (lift) stats_add(got.data(), lift->n_seq, stat_out->decay, stat_out->seq_cis, stat_out->seq_trans, stat_out->unlifted);
    for (int64_t q = 0; q < n_split; q++) split_out[q] += got_split[(size_t)q];
    return HICMI_OK;
}

int hicmi_build_maps(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names, const int64_t* scaf_size,
                     int64_t n_res, const int64_t* resolution, hicmi_ctx* const* ctxs, int threads, int64_t* stats5)
{
    return build_maps_loop(path, names_blob, name_off, n_names, scaf_size, n_res, resolution, ctxs, threads, stats5, nullptr, nullptr);
}

int hicmi_lift_maps(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names, const int64_t* scaf_size,
                    const int32_t* lift_seq, const int64_t* lift_off, const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq,
                    int64_t n_res, const int64_t* resolution, hicmi_ctx* const* ctxs, int threads, int64_t* stats5,
                    uint64_t* decay_out, uint64_t* seq_cis_out, uint64_t* seq_trans_out, uint64_t* unlifted_out)
{
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    const LiftStatsOut out{decay_out, seq_cis_out, seq_trans_out, unlifted_out};
    return build_maps_loop(path, names_blob, name_off, n_names, scaf_size, n_res, resolution, ctxs, threads, stats5, &lift, &out);
}

// hicmi_build_maps on the pieces the scaffolds are cut into: the parser reads the scaffolds' coordinates
int hicmi_split_maps(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names, const int64_t* scaf_size,
                     const int32_t* piece_first, const int64_t* piece_start, int64_t n_piece, int64_t n_res, const int64_t* resolution,
                     hicmi_ctx* const* ctxs, int threads, int64_t* stats5, uint64_t* counters_out)
{
    const SplitHost split{piece_first, piece_start, n_piece};
    return build_maps_loop(path, names_blob, name_off, n_names, scaf_size, n_res, resolution, ctxs, threads, stats5, nullptr, nullptr,
                           &split, counters_out);
}

// ---- spanning depth: the read pairs with one end on each side of every cell boundary ---------------------
// Between hicmi_span_begin and hicmi_span_finish the marks live in buffers of their own: the context's matrix state and
// an open map build are never touched (the staging of a chunk, d_map_chunk, holds nothing between calls).
static void span_abandon(hicmi_ctx* c)
{
    c->span_marks.reset(); c->d_span_lift.reset(); c->d_span_first.reset();
    c->span_lift = LiftTables(); c->span_grid = SpanGrid();
    c->span_size.clear(); c->span_seq_first.clear();
    c->span_pairs = 0;
}

// HICMI_SPANS_PLAIN: "1" two atomic adds per marking pair, "0" the combining kernel, anything else the default; read per call
constexpr bool kSpansPlainByDefault = false;
static bool spans_plain()
{
    return plain_switch(getenv("HICMI_SPANS_PLAIN"), kSpansPlainByDefault);
}

// the numbering of a build, made on the host before anything is allocated
struct SpanCells { std::vector<int64_t> cell_first, seq_first; int64_t n_cells = 0; };

static int span_number(const int64_t* scaf_size, int64_t n_scaf, const LiftHost& lift, int64_t step, int64_t max_span, SpanCells* out)
{
    if (!scaf_size || n_scaf < 1 || n_scaf > INT_MAX / 2) return fail(HICMI_EINVAL, "bad arguments");
    if (step < 1) return fail(HICMI_EINVAL, "step %lld is below 1", (long long)step);
    if (max_span < 0) return fail(HICMI_EINVAL, "max_span %lld is negative", (long long)max_span);
    int rc = lift_check(scaf_size, n_scaf, lift);
    if (rc) return rc;
    out->cell_first.resize((size_t)n_scaf);
    out->seq_first.resize((size_t)lift.n_seq + 1);
    out->n_cells = span_number_cells(scaf_size, n_scaf, lift.seq, lift.off, lift.n_seq, step, out->cell_first.data(), out->seq_first.data());
    if (out->n_cells < 0)
        return fail(HICMI_EUNSUPPORTED, "step %lld cuts the assembly into more than %lld cells", (long long)step, (long long)SPAN_MAX_CELLS);
    if (out->n_cells < 1) return fail(HICMI_EINVAL, "no scaffold with a base is placed: there are no cells");
    return HICMI_OK;
}

static int span_open(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const LiftHost& lift, int64_t step, int64_t max_span,
                     SpanCells&& cells)
{
    HIPCHK(hipSetDevice(c->device));
    span_abandon(c);                                          // a begin without a finish is given up
    const int64_t m = cells.n_cells;
    int rc = ensure_all(c->span_marks, m + SPAN_COUNTERS, c->d_span_first, n_scaf, c->d_span_lift, 21 * n_scaf);
    if (rc) return rc;
    rc = upload(c, c->d_span_first, cells.cell_first.data(), sizeof(int64_t) * (size_t)n_scaf);
    if (!rc) rc = lift_upload(c, c->d_span_lift, scaf_size, n_scaf, lift, &c->span_lift);
    if (!rc) rc = zero_and_wait(c, c->span_marks, sizeof(uint64_t) * (size_t)(m + SPAN_COUNTERS));
    if (rc) { span_abandon(c); return rc; }
    c->span_grid.cell_first = c->d_span_first; c->span_grid.step = step; c->span_grid.max_span = max_span; c->span_grid.n_cells = m;
    c->span_size.assign(scaf_size, scaf_size + n_scaf);
    c->span_seq_first = std::move(cells.seq_first);
    c->span_pairs = 0;
    return HICMI_OK;
}

// the flank and the records of a finish against the open build: nothing on the device is looked at
static int span_check_records(const hicmi_ctx* c, int64_t flank, const int64_t* recs, int64_t n_rec)
{
    if (flank < 1 || flank > SPAN_MAX_FLANK)
        return fail(HICMI_EINVAL, "flank %lld outside 1 .. %lld", (long long)flank, (long long)SPAN_MAX_FLANK);
    if (n_rec < 0 || n_rec > INT_MAX / 2 || (n_rec > 0 && !recs)) return fail(HICMI_EINVAL, "bad arguments");
    const std::vector<int64_t>& first = c->span_seq_first;
    for (int64_t r = 0; r < n_rec; r++) {
        const int64_t lo = recs[4 * r], hi = recs[4 * r + 1], q0 = recs[4 * r + 2], q1 = recs[4 * r + 3];
        // the last sequence that starts at or before q0 is the one that has cells there
        const size_t q = (size_t)(std::upper_bound(first.begin(), first.end(), q0) - first.begin());
        if (q0 < 0 || q == 0 || q >= first.size() || first[q - 1] != q0 || first[q] != q1 || lo < q0 || hi < lo || hi >= q1)
            return fail(HICMI_EINVAL, "record %lld (slots %lld .. %lld of the cells %lld .. %lld) is not a slot range inside one sequence",
                        (long long)r, (long long)lo, (long long)hi, (long long)q0, (long long)q1);
    }
    return HICMI_OK;
}

// the two scans, the picks and the downloads of an open build, which it closes; an output is written only when all are down
static int span_close(hicmi_ctx* c, int64_t flank, const int64_t* recs, int64_t n_rec, int64_t* picks_out, uint64_t* counters5_out,
                      uint64_t* depth_out)
{
    const int64_t m = c->span_grid.n_cells;
    if (c->span_pairs > (((int64_t)1 << 53) - 1) / flank) {
        span_abandon(c);
        return fail(HICMI_EUNSUPPORTED, "%lld pairs at a flank of %lld: depth x flank could reach 2^53", (long long)c->span_pairs,
                    (long long)flank);
    }
    struct Close { hicmi_ctx* c; ~Close() { span_abandon(c); } } closing{c};
    DevBuf<unsigned long long> d_depth, d_sums, d_tiles;
    DevBuf<int64_t> d_recs;                                   // [records][picks]
    int rc = ensure_all(d_depth, m, d_sums, m, d_tiles, span_scan_tiles(m), d_recs, 8 * n_rec);
    if (!rc && n_rec) rc = upload(c, d_recs, recs, sizeof(int64_t) * 4 * (size_t)n_rec);
    if (rc) return rc;
    launch_span_scan(c->span_marks, d_depth, m, d_tiles, c->stream);
    launch_span_scan(d_depth, d_sums, m, d_tiles, c->stream);
    launch_span_pick(d_depth, d_sums, m, flank, d_recs, n_rec, d_recs + 4 * n_rec, c->stream);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> picks((size_t)(4 * n_rec));
    uint64_t counters[SPAN_COUNTERS];
    rc = download(c, counters, c->span_marks + m, sizeof(counters));
    if (!rc && n_rec) rc = download(c, picks.data(), d_recs + 4 * n_rec, sizeof(int64_t) * picks.size());
    if (!rc && depth_out) {
        HIPCHK(hipMemcpyAsync(depth_out, d_depth, sizeof(uint64_t) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_stream(c));
    }
    if (rc) return rc;
    if (n_rec) memcpy(picks_out, picks.data(), sizeof(int64_t) * picks.size());
    memcpy(counters5_out, counters, sizeof(counters));
    return HICMI_OK;
}

int hicmi_span_begin(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                     const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, int64_t step, int64_t max_span,
                     int64_t* cell_first_out, int64_t* n_cells_out)
{
    if (!c || !cell_first_out || !n_cells_out) return fail(HICMI_EINVAL, "bad arguments");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    SpanCells cells;
    int rc = span_number(scaf_size, n_scaf, lift, step, max_span, &cells);
    if (rc) return rc;
    const std::vector<int64_t> cell_first = cells.cell_first;
    const int64_t m = cells.n_cells;
    rc = span_open(c, scaf_size, n_scaf, lift, step, max_span, std::move(cells));
    if (rc) return rc;
    memcpy(cell_first_out, cell_first.data(), sizeof(int64_t) * (size_t)n_scaf);
    *n_cells_out = m;
    return HICMI_OK;
}

int hicmi_span_add_pairs(hicmi_ctx* c, const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b,
                         int64_t n)
{
    if (!c || n < 0 || (n > 0 && (!scaf_a || !pos_a || !scaf_b || !pos_b))) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->span_marks) return fail(HICMI_EINVAL, "hicmi_span_add_pairs without hicmi_span_begin");
    int rc_pairs = check_pairs(scaf_a, pos_a, scaf_b, pos_b, n, c->span_size.data(), (int64_t)c->span_size.size(), nullptr, nullptr);
    if (rc_pairs) return rc_pairs;
    if (n == 0) return HICMI_OK;
    HIPCHK(hipSetDevice(c->device));
    // a HIP error from here on gives the build up: what was marked so far cannot be told
    MapChunk k;
    int rc = stage_chunk(c, scaf_a, pos_a, scaf_b, pos_b, n, &k);
    if (!rc) {
        launch_span_mark(k.scaf_a, k.pos_a, k.scaf_b, k.pos_b, n, c->span_lift, c->span_grid, c->span_marks,
                         c->span_marks + c->span_grid.n_cells, spans_plain(), c->stream);
        rc = wait_launched(c, "marking a chunk of pairs");
    }
    if (rc) { span_abandon(c); return rc; }
    c->span_pairs += n;
    return HICMI_OK;
}

int hicmi_span_finish(hicmi_ctx* c, int64_t flank, const int64_t* recs, int64_t n_rec, int64_t* picks_out, uint64_t* counters5_out,
                      uint64_t* depth_out)
{
    if (!c || !counters5_out || (n_rec > 0 && !picks_out)) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->span_marks) return fail(HICMI_EINVAL, "hicmi_span_finish without hicmi_span_begin");
    int rc = span_check_records(c, flank, recs, n_rec);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    return span_close(c, flank, recs, n_rec, picks_out, counters5_out, depth_out);
}

// The same over the pair file in one pass: pair_file_pass with the marks of one build.
int hicmi_span_file(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names, const int64_t* scaf_size,
                    const int32_t* lift_seq, const int64_t* lift_off, const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq,
                    int64_t step, int64_t max_span, int64_t flank, const int64_t* recs, int64_t n_rec, hicmi_ctx* c, int threads,
                    int64_t* stats5, int64_t* picks_out, uint64_t* counters5_out, uint64_t* depth_out, int64_t* cell_first_out,
                    int64_t* n_cells_out)
{
    if (!path || !names_blob || !name_off || !scaf_size || !c || !stats5 || !counters5_out || !cell_first_out || !n_cells_out ||
        n_names < 1 || (n_rec > 0 && !picks_out))
        return fail(HICMI_EINVAL, "bad arguments");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    SpanCells cells;
    int rc = span_number(scaf_size, n_names, lift, step, max_span, &cells);
    if (rc) return rc;
    int64_t chunk_pairs = 0;
    rc = chunk_pairs_setting(&chunk_pairs);
    if (rc) return rc;
    const std::vector<int64_t> cell_first = cells.cell_first;
    const int64_t m = cells.n_cells;
    rc = span_open(c, scaf_size, n_names, lift, step, max_span, std::move(cells));
    if (rc) return rc;
    struct OpenSpan { hicmi_ctx* c; bool keep = false; ~OpenSpan() { if (!keep) span_abandon(c); } } own{c};   // given up on every error path
    // the flank and the records are refused before the file is read
    rc = span_check_records(c, flank, recs, n_rec);
    if (rc) return rc;
    const bool plain = spans_plain();
    int64_t stats[5] = {0, 0, 0, 0, 0};
    rc = pair_file_pass(path, names_blob, name_off, n_names, scaf_size, c, threads, chunk_pairs, stats, "marking a chunk of pairs",
                        [&](const MapChunk& d, int64_t n) {
                            launch_span_mark(d.scaf_a, d.pos_a, d.scaf_b, d.pos_b, n, c->span_lift, c->span_grid, c->span_marks,
                                             c->span_marks + m, plain, c->stream);
                            c->span_pairs += n;
                        });
    if (rc) return rc;
    own.keep = true;                                               // span_close closes the build, whatever it returns
    rc = span_close(c, flank, recs, n_rec, picks_out, counters5_out, depth_out);
    if (rc) return rc;
    for (int k = 0; k < 5; k++) stats5[k] = stats[k];
    memcpy(cell_first_out, cell_first.data(), sizeof(int64_t) * (size_t)n_names);
    *n_cells_out = m;
    return HICMI_OK;
}

// ---- end support: the read pairs that link the ends of neighbouring scaffolds -----------------------------
// Between hicmi_ends_begin and hicmi_ends_finish the table lives in buffers of its own: the context's matrix state, an
// open map build and an open span build are never touched (the staging of a chunk, d_map_chunk, holds nothing between calls).
static void ends_abandon(hicmi_ctx* c)
{
    c->ends_table.reset(); c->d_ends_lift.reset(); c->d_ends_rank.reset();
    c->ends_lift = LiftTables(); c->ends_grid = EndsGrid();
    c->ends_size.clear();
    c->ends_cells = 0;
}

// HICMI_ENDS_PLAIN: "1" one atomic add per linked pair, "0" the combining kernel, anything else the default; read per call
constexpr bool kEndsPlainByDefault = false;
static bool ends_plain()
{
    return plain_switch(getenv("HICMI_ENDS_PLAIN"), kEndsPlainByDefault);
}

// the ranks of a build, made on the host before anything is allocated
struct EndsRanks { std::vector<int32_t> rank; int64_t n_placed = 0; };

static int ends_number(const int64_t* scaf_size, int64_t n_scaf, const LiftHost& lift, int64_t window, int64_t reach, EndsRanks* out)
{
    if (!scaf_size || n_scaf < 1 || n_scaf > INT_MAX / 2) return fail(HICMI_EINVAL, "bad arguments");
    if (window < 1) return fail(HICMI_EINVAL, "window %lld is below 1", (long long)window);
    if (reach < 1 || reach > ENDS_MAX_REACH)
        return fail(HICMI_EINVAL, "reach %lld outside 1 .. %lld", (long long)reach, (long long)ENDS_MAX_REACH);
    int rc = lift_check(scaf_size, n_scaf, lift);
    if (rc) return rc;
    out->rank.resize((size_t)n_scaf);
    std::vector<int64_t> seq_first((size_t)lift.n_seq + 1);
    out->n_placed = ends_number_ranks(scaf_size, n_scaf, lift.seq, lift.off, lift.n_seq, reach, out->rank.data(), seq_first.data());
    if (out->n_placed < 0)
        return fail(HICMI_EUNSUPPORTED, "reach %lld over the placed scaffolds needs a table of more than %lld counters", (long long)reach,
                    (long long)ENDS_MAX_TABLE);
    if (out->n_placed < 1) return fail(HICMI_EINVAL, "no scaffold with a base is placed: there are no ends");
    return HICMI_OK;
}

static int ends_open(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const LiftHost& lift, int64_t window, int64_t reach,
                     const EndsRanks& ranks)
{
    HIPCHK(hipSetDevice(c->device));
    ends_abandon(c);                                          // a begin without a finish is given up
    const int64_t m = ranks.n_placed * reach * 4;
    int rc = ensure_all(c->ends_table, m + ENDS_COUNTERS, c->d_ends_rank, n_scaf, c->d_ends_lift, 21 * n_scaf);
    if (rc) return rc;
    rc = upload(c, c->d_ends_rank, ranks.rank.data(), sizeof(int32_t) * (size_t)n_scaf);
    if (!rc) rc = lift_upload(c, c->d_ends_lift, scaf_size, n_scaf, lift, &c->ends_lift);
    if (!rc) rc = zero_and_wait(c, c->ends_table, sizeof(uint64_t) * (size_t)(m + ENDS_COUNTERS));
    if (rc) { ends_abandon(c); return rc; }
    c->ends_grid.rank = c->d_ends_rank; c->ends_grid.window = window; c->ends_grid.reach = reach; c->ends_grid.n_placed = ranks.n_placed;
    c->ends_size.assign(scaf_size, scaf_size + n_scaf);
    c->ends_cells = m;
    return HICMI_OK;
}

// the downloads of an open build, which it closes; the counters are written only when the table is down
static int ends_close(hicmi_ctx* c, uint64_t* table_out, uint64_t* counters6_out)
{
    struct Close { hicmi_ctx* c; ~Close() { ends_abandon(c); } } closing{c};
    return download_table(c, c->ends_table, c->ends_cells, ENDS_COUNTERS, table_out, counters6_out);
}

int hicmi_ends_begin(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                     const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, int64_t window, int64_t reach,
                     int32_t* rank_out, int64_t* n_placed_out)
{
    if (!c || !rank_out || !n_placed_out) return fail(HICMI_EINVAL, "bad arguments");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    EndsRanks ranks;
    int rc = ends_number(scaf_size, n_scaf, lift, window, reach, &ranks);
    if (rc) return rc;
    rc = ends_open(c, scaf_size, n_scaf, lift, window, reach, ranks);
    if (rc) return rc;
    memcpy(rank_out, ranks.rank.data(), sizeof(int32_t) * (size_t)n_scaf);
    *n_placed_out = ranks.n_placed;
    return HICMI_OK;
}

int hicmi_ends_add_pairs(hicmi_ctx* c, const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b,
                         int64_t n)
{
    if (!c || n < 0 || (n > 0 && (!scaf_a || !pos_a || !scaf_b || !pos_b))) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->ends_table) return fail(HICMI_EINVAL, "hicmi_ends_add_pairs without hicmi_ends_begin");
    int rc_pairs = check_pairs(scaf_a, pos_a, scaf_b, pos_b, n, c->ends_size.data(), (int64_t)c->ends_size.size(), nullptr, nullptr);
    if (rc_pairs) return rc_pairs;
    if (n == 0) return HICMI_OK;
    HIPCHK(hipSetDevice(c->device));
    // a HIP error from here on gives the build up: what was counted so far cannot be told
    MapChunk k;
    int rc = stage_chunk(c, scaf_a, pos_a, scaf_b, pos_b, n, &k);
    if (!rc) {
        launch_ends_count(k.scaf_a, k.pos_a, k.scaf_b, k.pos_b, n, c->ends_lift, c->ends_grid, c->ends_cells, c->ends_table,
                          c->ends_table + c->ends_cells, ends_plain(), c->stream);
        rc = wait_launched(c, "counting a chunk of pairs");
    }
    if (rc) { ends_abandon(c); return rc; }
    return HICMI_OK;
}

int hicmi_ends_finish(hicmi_ctx* c, uint64_t* table_out, uint64_t* counters6_out)
{
    if (!c || !table_out || !counters6_out) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->ends_table) return fail(HICMI_EINVAL, "hicmi_ends_finish without hicmi_ends_begin");
    HIPCHK(hipSetDevice(c->device));
    return ends_close(c, table_out, counters6_out);
}

// The same over the pair file in one pass: pair_file_pass with the table of one build.
int hicmi_ends_file(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names, const int64_t* scaf_size,
                    const int32_t* lift_seq, const int64_t* lift_off, const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq,
                    int64_t window, int64_t reach, hicmi_ctx* c, int threads, int64_t* stats5, uint64_t* table_out,
                    uint64_t* counters6_out, int32_t* rank_out, int64_t* n_placed_out)
{
    if (!path || !names_blob || !name_off || !scaf_size || !c || !stats5 || !table_out || !counters6_out || !rank_out || !n_placed_out ||
        n_names < 1)
        return fail(HICMI_EINVAL, "bad arguments");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    EndsRanks ranks;
    int rc = ends_number(scaf_size, n_names, lift, window, reach, &ranks);
    if (rc) return rc;
    int64_t chunk_pairs = 0;
    rc = chunk_pairs_setting(&chunk_pairs);
    if (rc) return rc;
    rc = ends_open(c, scaf_size, n_names, lift, window, reach, ranks);
    if (rc) return rc;
    struct OpenEnds { hicmi_ctx* c; bool keep = false; ~OpenEnds() { if (!keep) ends_abandon(c); } } own{c};   // given up on every error path
    const bool plain = ends_plain();
    int64_t stats[5] = {0, 0, 0, 0, 0};
    rc = pair_file_pass(path, names_blob, name_off, n_names, scaf_size, c, threads, chunk_pairs, stats, "counting a chunk of pairs",
                        [&](const MapChunk& d, int64_t n) {
                            launch_ends_count(d.scaf_a, d.pos_a, d.scaf_b, d.pos_b, n, c->ends_lift, c->ends_grid, c->ends_cells,
                                              c->ends_table, c->ends_table + c->ends_cells, plain, c->stream);
                        });
    if (rc) return rc;
    // the table comes down into memory of the library's first: an error after it leaves every output as it was
    std::vector<uint64_t> table((size_t)c->ends_cells);
    uint64_t counters[ENDS_COUNTERS];
    own.keep = true;                                               // ends_close closes the build, whatever it returns
    rc = ends_close(c, table.data(), counters);
    if (rc) return rc;
    memcpy(table_out, table.data(), sizeof(uint64_t) * table.size());
    memcpy(counters6_out, counters, sizeof(counters));
    for (int k = 0; k < 5; k++) stats5[k] = stats[k];
    memcpy(rank_out, ranks.rank.data(), sizeof(int32_t) * (size_t)n_names);
    *n_placed_out = ranks.n_placed;
    return HICMI_OK;
}

// ---- anchoring: the read pairs that link the scaffolds an ordering leaves out to the placed ones -----------
// Between hicmi_anchor_begin and hicmi_anchor_finish the table lives in buffers of its own: the context's matrix state, an
// open map build, an open span build and an open ends build are never touched (the staging of a chunk, d_map_chunk, holds
// nothing between calls).
static void anchor_abandon(hicmi_ctx* c)
{
    c->anchor_table.reset(); c->d_anchor_lift.reset(); c->d_anchor_first.reset(); c->d_anchor_target.reset();
    c->anchor_lift = LiftTables(); c->anchor_grid = AnchorGrid();
    c->anchor_size.clear();
    c->anchor_cells = 0;
}

// HICMI_ANCHOR_PLAIN: "1" one atomic add per anchored pair, "0" the combining kernel, anything else the default; read per call
constexpr bool kAnchorPlainByDefault = false;
static bool anchor_plain()
{
    return plain_switch(getenv("HICMI_ANCHOR_PLAIN"), kAnchorPlainByDefault);
}

// the blocks of a build, made on the host before anything is allocated
struct AnchorBlocks { std::vector<int64_t> first, seq_first; std::vector<int32_t> rank; int64_t n_table = 0; };

static int anchor_number(const int64_t* scaf_size, int64_t n_scaf, const LiftHost& lift, const int32_t* target, int64_t window,
                         AnchorBlocks* out)
{
    if (!scaf_size || n_scaf < 1 || n_scaf > INT_MAX / 2) return fail(HICMI_EINVAL, "bad arguments");
    if (window < 1) return fail(HICMI_EINVAL, "window %lld is below 1", (long long)window);
    int rc = lift_check(scaf_size, n_scaf, lift);
    if (rc) return rc;
    out->first.resize((size_t)n_scaf);
    out->seq_first.assign((size_t)lift.n_seq + 1, 0);
    if (target) {
        out->rank.resize((size_t)n_scaf);
        if (ends_number_ranks(scaf_size, n_scaf, lift.seq, lift.off, lift.n_seq, 1, out->rank.data(), out->seq_first.data()) < 0)
            return fail(HICMI_EUNSUPPORTED, "more than %lld placed scaffolds", (long long)(ENDS_MAX_TABLE / 4));
        char msg[256];
        if (anchor_check_targets(scaf_size, n_scaf, lift.seq, lift.n_seq, target, out->seq_first.data(), msg, sizeof(msg)))
            return fail(HICMI_EINVAL, "%s", msg);
    }
    out->n_table = anchor_number_blocks(scaf_size, n_scaf, lift.seq, lift.n_seq, target, out->seq_first.data(), out->first.data());
    if (out->n_table < 0)
        return fail(HICMI_EUNSUPPORTED, "the candidates need a table of more than %lld counters", (long long)ANCHOR_MAX_TABLE);
    if (out->n_table < 1)
        return fail(HICMI_EINVAL, target ? "no scaffold has a target: there is no candidate"
                                         : "every scaffold with a base is placed: there is no candidate");
    return HICMI_OK;
}

static int anchor_open(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const LiftHost& lift, const int32_t* target,
                       int64_t window, const AnchorBlocks& blocks)
{
    HIPCHK(hipSetDevice(c->device));
    anchor_abandon(c);                                        // a begin without a finish is given up
    const int64_t m = blocks.n_table, n_first = n_scaf + lift.n_seq + 1;
    int rc = ensure_all(c->anchor_table, m + ANCHOR_COUNTERS, c->d_anchor_first, n_first, c->d_anchor_target, target ? 2 * n_scaf : 1,
                        c->d_anchor_lift, 21 * n_scaf);
    if (rc) return rc;
    rc = upload(c, c->d_anchor_first, blocks.first.data(), sizeof(int64_t) * (size_t)n_scaf);
    if (!rc) rc = upload(c, c->d_anchor_first + n_scaf, blocks.seq_first.data(), sizeof(int64_t) * (size_t)(lift.n_seq + 1));
    if (!rc && target) rc = upload(c, c->d_anchor_target, target, sizeof(int32_t) * (size_t)n_scaf);
    if (!rc && target) rc = upload(c, c->d_anchor_target + n_scaf, blocks.rank.data(), sizeof(int32_t) * (size_t)n_scaf);
    if (!rc) rc = lift_upload(c, c->d_anchor_lift, scaf_size, n_scaf, lift, &c->anchor_lift);
    if (!rc) rc = zero_and_wait(c, c->anchor_table, sizeof(uint64_t) * (size_t)(m + ANCHOR_COUNTERS));
    if (rc) { anchor_abandon(c); return rc; }
    c->anchor_grid.first = c->d_anchor_first; c->anchor_grid.seq_first = c->d_anchor_first + n_scaf;
    c->anchor_grid.target = target ? (const int32_t*)c->d_anchor_target : nullptr;
    c->anchor_grid.rank = target ? c->d_anchor_target + n_scaf : nullptr;
    c->anchor_grid.window = window;
    c->anchor_size.assign(scaf_size, scaf_size + n_scaf);
    c->anchor_cells = m;
    return HICMI_OK;
}

// the downloads of an open build, which it closes; the counters are written only when the table is down
static int anchor_close(hicmi_ctx* c, uint64_t* table_out, uint64_t* counters6_out)
{
    struct Close { hicmi_ctx* c; ~Close() { anchor_abandon(c); } } closing{c};
    return download_table(c, c->anchor_table, c->anchor_cells, ANCHOR_COUNTERS, table_out, counters6_out);
}

int hicmi_anchor_begin(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                       const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, const int32_t* target, int64_t window,
                       int64_t* first_out, int64_t* n_table_out)
{
    if (!c || !first_out || !n_table_out) return fail(HICMI_EINVAL, "bad arguments");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    AnchorBlocks blocks;
    int rc = anchor_number(scaf_size, n_scaf, lift, target, window, &blocks);
    if (rc) return rc;
    rc = anchor_open(c, scaf_size, n_scaf, lift, target, window, blocks);
    if (rc) return rc;
    memcpy(first_out, blocks.first.data(), sizeof(int64_t) * (size_t)n_scaf);
    *n_table_out = blocks.n_table;
    return HICMI_OK;
}

int hicmi_anchor_add_pairs(hicmi_ctx* c, const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b,
                           int64_t n)
{
    if (!c || n < 0 || (n > 0 && (!scaf_a || !pos_a || !scaf_b || !pos_b))) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->anchor_table) return fail(HICMI_EINVAL, "hicmi_anchor_add_pairs without hicmi_anchor_begin");
    int rc_pairs = check_pairs(scaf_a, pos_a, scaf_b, pos_b, n, c->anchor_size.data(), (int64_t)c->anchor_size.size(), nullptr, nullptr);
    if (rc_pairs) return rc_pairs;
    if (n == 0) return HICMI_OK;
    HIPCHK(hipSetDevice(c->device));
    // a HIP error from here on gives the build up: what was counted so far cannot be told
    MapChunk k;
    int rc = stage_chunk(c, scaf_a, pos_a, scaf_b, pos_b, n, &k);
    if (!rc) {
        launch_anchor_count(k.scaf_a, k.pos_a, k.scaf_b, k.pos_b, n, c->anchor_lift, c->anchor_grid, c->anchor_cells, c->anchor_table,
                            c->anchor_table + c->anchor_cells, anchor_plain(), c->stream);
        rc = wait_launched(c, "counting a chunk of pairs");
    }
    if (rc) { anchor_abandon(c); return rc; }
    return HICMI_OK;
}

int hicmi_anchor_finish(hicmi_ctx* c, uint64_t* table_out, uint64_t* counters6_out)
{
    if (!c || !table_out || !counters6_out) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->anchor_table) return fail(HICMI_EINVAL, "hicmi_anchor_finish without hicmi_anchor_begin");
    HIPCHK(hipSetDevice(c->device));
    return anchor_close(c, table_out, counters6_out);
}

// The same over the pair file in one pass: pair_file_pass with the table of one build.
int hicmi_anchor_file(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names, const int64_t* scaf_size,
                      const int32_t* lift_seq, const int64_t* lift_off, const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq,
                      const int32_t* target, int64_t window, hicmi_ctx* c, int threads, int64_t* stats5, uint64_t* table_out,
                      uint64_t* counters6_out, int64_t* first_out, int64_t* n_table_out)
{
    if (!path || !names_blob || !name_off || !scaf_size || !c || !stats5 || !table_out || !counters6_out || !first_out || !n_table_out ||
        n_names < 1)
        return fail(HICMI_EINVAL, "bad arguments");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    AnchorBlocks blocks;
    int rc = anchor_number(scaf_size, n_names, lift, target, window, &blocks);
    if (rc) return rc;
    int64_t chunk_pairs = 0;
    rc = chunk_pairs_setting(&chunk_pairs);
    if (rc) return rc;
    rc = anchor_open(c, scaf_size, n_names, lift, target, window, blocks);
    if (rc) return rc;
    struct OpenAnchor { hicmi_ctx* c; bool keep = false; ~OpenAnchor() { if (!keep) anchor_abandon(c); } } own{c};   // given up on every error path
    const bool plain = anchor_plain();
    int64_t stats[5] = {0, 0, 0, 0, 0};
    rc = pair_file_pass(path, names_blob, name_off, n_names, scaf_size, c, threads, chunk_pairs, stats, "counting a chunk of pairs",
                        [&](const MapChunk& d, int64_t n) {
                            launch_anchor_count(d.scaf_a, d.pos_a, d.scaf_b, d.pos_b, n, c->anchor_lift, c->anchor_grid, c->anchor_cells,
                                                c->anchor_table, c->anchor_table + c->anchor_cells, plain, c->stream);
                        });
    if (rc) return rc;
    // the table comes down into memory of the library's first: an error after it leaves every output as it was
    std::vector<uint64_t> table((size_t)c->anchor_cells);
    uint64_t counters[ANCHOR_COUNTERS];
    own.keep = true;                                               // anchor_close closes the build, whatever it returns
    rc = anchor_close(c, table.data(), counters);
    if (rc) return rc;
    memcpy(table_out, table.data(), sizeof(uint64_t) * table.size());
    memcpy(counters6_out, counters, sizeof(counters));
    for (int k = 0; k < 5; k++) stats5[k] = stats[k];
    memcpy(first_out, blocks.first.data(), sizeof(int64_t) * (size_t)n_names);
    *n_table_out = blocks.n_table;
    return HICMI_OK;
}

// ---- the resident pair store: hicmi_pairs_*, hicmi_ends_resident, hicmi_anchor_resident --------------------
#include "api_pairs.inc"

// ---- the end-link graph on lifted ends: hicmi_links_lifted, on the store and the rows of the calls above ----
#include "api_links.inc"

// Group support: extends the scaffold vote of assessChromosomeClustering (S2C:1001-1077) with the
// contacts themselves.  The host sorts the grouped rows by group and cuts them into chunks of GS_CHUNK; the kernels of
// k_group_support.hip read every grouped row once.
int hicmi_group_sums(hicmi_ctx* c, const int32_t* grp, const int32_t* scaf, int64_t n_groups, int64_t n_scaffolds,
                     double* bin_sums_out, double* scaffold_sums_out)
{
    if (!c || !grp || !scaf || !scaffold_sums_out) return fail(HICMI_EINVAL, "NULL argument");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    if (n_groups < 1 || n_groups > 65536) return fail(HICMI_EINVAL, "n_groups = %lld outside 1 .. 65536", (long long)n_groups);
    if (n_scaffolds < 1 || n_scaffolds > INT_MAX / 2) return fail(HICMI_EINVAL, "n_scaffolds = %lld out of range", (long long)n_scaffolds);
    const int64_t n = c->n, G = n_groups, S = n_scaffolds;
    std::vector<int32_t> gcount(G + 1, 0), soff(S + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        if (grp[i] < -1 || grp[i] >= G) return fail(HICMI_EINVAL, "grp[%lld] = %d outside -1 .. %lld", (long long)i, grp[i], (long long)(G - 1));
        if (scaf[i] < 0 || scaf[i] >= S) return fail(HICMI_EINVAL, "scaf[%lld] = %d outside 0 .. %lld", (long long)i, scaf[i], (long long)(S - 1));
        if (grp[i] >= 0) gcount[grp[i] + 1]++;
        soff[scaf[i] + 1]++;
    }
    for (int64_t g = 0; g < G; g++) gcount[g + 1] += gcount[g];
    for (int64_t s = 0; s < S; s++) soff[s + 1] += soff[s];
    const int64_t R = gcount[G];
    // one host image of every list: [chunks][rows][group_chunk0][scaf][sbins][soff]
    std::vector<GsChunk> chunks;
    std::vector<int32_t> gc0(G + 1, 0);
    for (int64_t g = 0; g < G; g++) {
        gc0[g] = (int32_t)chunks.size();
        for (int32_t r0 = gcount[g]; r0 < gcount[g + 1]; r0 += GS_CHUNK)
            chunks.push_back({r0, std::min<int32_t>(GS_CHUNK, gcount[g + 1] - r0), (int32_t)g, 0});
    }
    gc0[G] = (int32_t)chunks.size();
    const int64_t NC = (int64_t)chunks.size();
    const int64_t o_rows = 4 * NC, o_gc0 = o_rows + R, o_scaf = o_gc0 + G + 1, o_sbins = o_scaf + n, o_soff = o_sbins + n,
                  n_ints = o_soff + S + 1;
    std::vector<int32_t> img((size_t)n_ints);
    if (NC) memcpy(img.data(), chunks.data(), sizeof(GsChunk) * (size_t)NC);
    {
        std::vector<int32_t> gfill(gcount.begin(), gcount.end() - 1), sfill(soff.begin(), soff.end() - 1);
        for (int64_t i = 0; i < n; i++) {                  // ascending i: ascending rows inside a group, bin-list order inside a scaffold
            if (grp[i] >= 0) img[(size_t)(o_rows + gfill[grp[i]]++)] = (int32_t)i;
            img[(size_t)(o_sbins + sfill[scaf[i]]++)] = (int32_t)i;
        }
    }
    memcpy(&img[(size_t)o_gc0], gc0.data(), sizeof(int32_t) * (size_t)(G + 1));
    memcpy(&img[(size_t)o_scaf], scaf, sizeof(int32_t) * (size_t)n);
    memcpy(&img[(size_t)o_soff], soff.data(), sizeof(int32_t) * (size_t)(S + 1));
    const bool plain = plain_switch(getenv("HICMI_GROUP_SUPPORT_PLAIN"), false);
    HIPCHK(hipSetDevice(c->device));
    const int64_t o_bin = plain ? 0 : NC * n, o_sc = o_bin + n * G, n_dbl = o_sc + S * G;
    int rc = ensure(c->d_gs_lists, n_ints);
    if (!rc) rc = ensure(c->d_gs_sums, n_dbl);
    if (!rc) rc = upload(c, c->d_gs_lists, img.data(), sizeof(int32_t) * (size_t)n_ints);
    if (rc) return rc;
    const int32_t* L = c->d_gs_lists;
    launch_group_sums(c->dC, c->ldc, (int)n, (int)G, (int)S, L + o_rows, reinterpret_cast<const GsChunk*>(L), (int)NC, L + o_gc0,
                      L + o_scaf, L + o_sbins, L + o_soff, c->d_gs_sums, c->d_gs_sums + o_bin, c->d_gs_sums + o_sc, plain,
                      c->stream);
    HIPCHK(hipGetLastError());
    if (bin_sums_out) { rc = download(c, bin_sums_out, c->d_gs_sums + o_bin, sizeof(double) * (size_t)(n * G)); if (rc) return rc; }
    return download(c, scaffold_sums_out, c->d_gs_sums + o_sc, sizeof(double) * (size_t)(S * G));
}

// Junction support: extends the chromosome loop of orderGenome (OG:608-612), which orders every group on
// its own and never looks from one group at another.  The host checks every record and cuts the rows of A into slabs;
// the kernels of k_junctions.hip read the sides as views of `bins`.
int hicmi_junction_sums(hicmi_ctx* c, const int32_t* bins, int64_t n_listed, const int64_t* rec, int64_t n_rec,
                        double* sums_out)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    if (n_rec < 0 || n_listed < 0) return fail(HICMI_EINVAL, "negative count");
    if (n_rec == 0) return HICMI_OK;
    if (!bins || !rec || !sums_out) return fail(HICMI_EINVAL, "NULL argument");
    if (n_listed < 1 || n_listed > INT_MAX) return fail(HICMI_EINVAL, "n_listed = %lld outside 1 .. 2^31 - 1", (long long)n_listed);
    if (n_rec > INT_MAX) return fail(HICMI_EUNSUPPORTED, "n_rec = %lld above 2^31 - 1", (long long)n_rec);
    const int64_t n = c->n;
    for (int64_t i = 0; i < n_listed; i++)
        if (bins[i] < 0 || bins[i] >= n)
            return fail(HICMI_EINVAL, "bins[%lld] = %d outside 0 .. %lld", (long long)i, bins[i], (long long)(n - 1));
    std::vector<JnRec> recs((size_t)n_rec);
    int64_t n_wg = 0, max_d = 0;
    for (int64_t r = 0; r < n_rec; r++) {
        const int64_t* q = rec + 6 * r;
        for (int side = 0; side < 2; side++) {
            const int64_t start = q[3 * side], step = q[3 * side + 1], len = q[3 * side + 2];
            if (len < 1) return fail(HICMI_EINVAL, "record %lld: a side of %lld bins", (long long)r, (long long)len);
            if (step != 1 && step != -1) return fail(HICMI_EINVAL, "record %lld: step %lld is not +1 or -1", (long long)r, (long long)step);
            if (len > n_listed || start < 0 || start >= n_listed || start + (len - 1) * step < 0 || start + (len - 1) * step >= n_listed)
                return fail(HICMI_EINVAL, "record %lld: a side runs outside the %lld listed bins", (long long)r, (long long)n_listed);
        }
        JnRec& d = recs[(size_t)r];
        d.wg0 = n_wg;
        d.startA = (int32_t)q[0]; d.stepA = (int32_t)q[1]; d.lenA = (int32_t)q[2];
        d.startB = (int32_t)q[3]; d.stepB = (int32_t)q[4]; d.lenB = (int32_t)q[5];
        d.n_slabs = (d.lenA + JN_SLAB_ROWS - 1) / JN_SLAB_ROWS; d.pad = 0;
        n_wg += d.n_slabs;
        max_d = std::max<int64_t>(max_d, q[2] + q[5] - 1);
    }
    const bool plain = plain_switch(getenv("HICMI_JUNCTIONS_PLAIN"), false);
    if (!plain && n_wg > INT_MAX) return fail(HICMI_EUNSUPPORTED, "%lld workgroups: at most 2^31 - 1", (long long)n_wg);
    std::vector<double> w((size_t)max_d + 1);
    w[0] = 0.0;
    for (int64_t d = 1; d <= max_d; d++) w[(size_t)d] = 1.0 / (double)d;       // IEEE division: NumPy's 1.0 / d
    HIPCHK(hipSetDevice(c->device));
    const int64_t rec_bytes = (int64_t)sizeof(JnRec) * n_rec, list_bytes = rec_bytes + (int64_t)sizeof(int32_t) * n_listed;
    const int64_t o_part = max_d + 1, o_sums = o_part + (plain ? 0 : n_wg), n_dbl = o_sums + n_rec;
    int rc = ensure(c->d_jn_lists, list_bytes);
    if (!rc) rc = ensure(c->d_jn_sums, n_dbl);
    if (!rc) rc = upload(c, c->d_jn_lists, recs.data(), (size_t)rec_bytes);
    if (!rc) rc = upload(c, c->d_jn_lists + rec_bytes, bins, sizeof(int32_t) * (size_t)n_listed);
    if (!rc) rc = upload(c, c->d_jn_sums, w.data(), sizeof(double) * w.size());
    if (rc) return rc;
    launch_junction_sums(c->dC, c->ldc, reinterpret_cast<const int32_t*>(c->d_jn_lists + rec_bytes),
                         reinterpret_cast<const JnRec*>(c->d_jn_lists.get()), (int)n_rec, n_wg, c->d_jn_sums,
                         c->d_jn_sums + o_part, c->d_jn_sums + o_sums, plain, c->stream);
    HIPCHK(hipGetLastError());
    return download(c, sums_out, c->d_jn_sums + o_sums, sizeof(double) * (size_t)n_rec);
}

// ---- ICE balancing: HiC-Pro's `ice` step on the resident raw map -------------------------------------
namespace {
// the matrix has changed under everything derived from it
int ice_matrix_changed(hicmi_ctx* c)
{
    return forget_matrix_derived(c);
}

int ice_check(hicmi_ctx* c, const char* what)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    if (c->n > 65536) return fail(HICMI_EUNSUPPORTED, "n = %lld > 65536 bins", (long long)c->n);
    if (!c->own_c)
        return fail(HICMI_ESTATE, "%s rewrites the contact matrix: a matrix adopted with hicmi_set_contacts_device is the "
                                  "caller's and is not touched", what);
    return HICMI_OK;
}

int ice_upload_mask(hicmi_ctx* c, const uint8_t* mask)
{
    int rc = ensure(c->d_ice_mask, c->n);
    if (!rc) rc = upload(c, c->d_ice_mask, mask, (size_t)c->n);
    return rc;
}
}  // namespace

int hicmi_ice_mask_rows(hicmi_ctx* c, const uint8_t* mask, int64_t n)
{
    int rc = ice_check(c, "hicmi_ice_mask_rows");
    if (rc) return rc;
    if (!mask || n != c->n) return fail(HICMI_EINVAL, "mask must have n = %lld entries", (long long)c->n);
    HIPCHK(hipSetDevice(c->device));
    if ((rc = ice_matrix_changed(c))) return rc;
    if ((rc = ice_upload_mask(c, mask))) return rc;
    launch_ice_mask(c->dC, c->ldc, (int)c->n, c->d_ice_mask, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_ice_balance(hicmi_ctx* c, const uint8_t* mask, int64_t max_iter, double eps, double* bias_out, int64_t* iters_out,
                      double* delta_out)
{
    int rc = ice_check(c, "hicmi_ice_balance");
    if (rc) return rc;
    if (max_iter < 1 || max_iter > (1 << 20)) return fail(HICMI_EINVAL, "max_iter = %lld outside 1 .. 2^20", (long long)max_iter);
    if (!(eps >= 0.0)) return fail(HICMI_EINVAL, "eps must be >= 0");
    const bool inplace = plain_switch(getenv("HICMI_ICE_INPLACE"), false);
    HIPCHK(hipSetDevice(c->device));
    if ((rc = ice_matrix_changed(c))) return rc;
    const int n = (int)c->n;
    const int64_t np = ((int64_t)n + 1) & ~(int64_t)1;       // every vector starts 16-byte aligned
    if ((rc = ensure(c->d_ice, 7 * np + 2 + 2 * max_iter))) return rc;
    double *y = c->d_ice, *u = y + np, *bias = u + np, *prev = bias + np, *s = prev + np, *d = s + np, *ones = d + np,
           *st = ones + np, *rec = st + 2;
    if (mask) {
        if ((rc = ice_upload_mask(c, mask))) return rc;
        launch_ice_mask(c->dC, c->ldc, n, c->d_ice_mask, c->stream);
    }
    launch_ice_fill(u, (int)(4 * np), 1.0, c->stream);       // u, bias, bias_prev (and s)
    launch_ice_fill(ones, (int)np, 1.0, c->stream);
    // the raw map's row sums and mean0
    launch_ice_rowdot(c->dC, c->ldc, n, ones, y, c->stream);
    launch_ice_vec_b(n, y, nullptr, bias, prev, s, st, rec, 0, 1, c->stream);
    HIPCHK(hipGetLastError());
    int64_t iters = 0;
    double delta = NAN;
    for (int64_t it = 0; it < max_iter; it++) {
        if (inplace) {
            launch_ice_vec_a(n, y, bias, nullptr, d, c->stream);
            launch_ice_scale(c->dC, c->ldc, n, d, st, 0, c->stream);
            launch_ice_rowdot(c->dC, c->ldc, n, ones, y, c->stream);
            launch_ice_vec_b(n, y, nullptr, bias, prev, s, st, rec, (int)it, 0, c->stream);
            launch_ice_scale(c->dC, c->ldc, n, d, st, 1, c->stream);
            launch_ice_rowdot(c->dC, c->ldc, n, ones, y, c->stream);      // the next iteration's row sums
        } else {
            launch_ice_vec_a(n, s, bias, u, d, c->stream);
            launch_ice_rowdot(c->dC, c->ldc, n, u, y, c->stream);
            launch_ice_vec_b(n, y, u, bias, prev, s, st, rec, (int)it, 0, c->stream);
        }
        HIPCHK(hipGetLastError());
        double r[2];
        if ((rc = download(c, r, rec + 2 * it, sizeof(r)))) return rc;      // the one small record of this iteration
        iters = it + 1;
        if (it > 0) {
            delta = r[0];
            if (delta < eps) break;
        }
    }
    if (!inplace) {
        launch_ice_apply(c->dC, c->ldc, n, u, c->stream);
        HIPCHK(hipGetLastError());
    }
    if (bias_out) {
        if ((rc = download(c, bias_out, bias, sizeof(double) * (size_t)n))) return rc;
        if (mask)
            for (int i = 0; i < n; i++)
                if (mask[i]) bias_out[i] = NAN;
    } else HIPCHK(sync_stream(c));
    if (iters_out) *iters_out = iters;
    if (delta_out) *delta_out = delta;
    return HICMI_OK;
}

int hicmi_get_contact_rows(hicmi_ctx* c, int64_t row0, int64_t nrows, double* out)
{
    if (!c || !out) return fail(HICMI_EINVAL, "NULL argument");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    if (row0 < 0 || nrows < 0 || row0 + nrows > c->n) return fail(HICMI_EINVAL, "rows out of range");
    HIPCHK(hipSetDevice(c->device));
    const int64_t n = c->n;
    const int64_t block = std::max<int64_t>(1, ((int64_t)64 << 20) / (8 * n));      // rows per staged copy
    for (int64_t r = 0; r < nrows; r += block) {
        const int64_t cnt = std::min(block, nrows - r);
        const size_t bytes = sizeof(double) * (size_t)(cnt * n);
        int rc = ensure_pin_down(c, bytes);
        if (rc) return rc;
        HIPCHK(hipMemcpy2DAsync(c->pin_down, sizeof(double) * (size_t)n, c->dC + (row0 + r) * c->ldc, sizeof(double) * (size_t)c->ldc,
                                sizeof(double) * (size_t)n, (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_stream(c));
        memcpy(out + r * n, c->pin_down, bytes);
    }
    if (nrows == 0) HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_selftest_division(hicmi_ctx* c, uint64_t seed, int64_t samples, uint64_t* mismatches_out)
{
    if (!c || !mismatches_out || samples < 1) return fail(HICMI_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    DevBuf<unsigned long long> d;
    int rc = ensure(d, 1);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream));
    const int blocks = 2048, iters = (int)std::max<int64_t>(1, samples / (blocks * 256));
    launch_selftest_division(seed, blocks, iters, d, c->stream);
    HIPCHK(hipGetLastError());
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_stream(c));
    *mismatches_out = bad;
    return HICMI_OK;
}

// ---------------------------------------------------------------------------------------------------
int hicmi_label_linkage(const double* zraw, int64_t n, double* Z)
{
    if (!zraw || !Z || n < 1) return fail(HICMI_EINVAL, "bad arguments");
    const int64_t m = n - 1;
    // numpy argsort(kind='mergesort') on the heights: stable.  (height, index) pairs side by side: the comparator of an
    // index sort fetched two scattered heights per comparison - 1.1 ms at 16k bins, 6.3 ms at 64k
    std::vector<std::pair<double, int64_t>> keyed((size_t)m);
    for (int64_t i = 0; i < m; i++) keyed[(size_t)i] = {zraw[4 * i + 2], i};
    std::stable_sort(keyed.begin(), keyed.end(),
                     [](const std::pair<double, int64_t>& x, const std::pair<double, int64_t>& y) { return x.first < y.first; });
    std::vector<int64_t> idx((size_t)m);
    for (int64_t i = 0; i < m; i++) idx[(size_t)i] = keyed[(size_t)i].second;
    std::vector<int64_t> parent((size_t)(2 * n - 1)), sz((size_t)(2 * n - 1), 0);
    for (int64_t i = 0; i < 2 * n - 1; i++) { parent[i] = i; if (i < n) sz[i] = 1; }
    auto find = [&](int64_t x) {
        int64_t p = x;
        while (parent[x] != x) x = parent[x];
        while (parent[p] != x) { int64_t nx = parent[p]; parent[p] = x; p = nx; }
        return x;
    };
    int64_t next = n;
    for (int64_t r = 0; r < m; r++) {
        const double* s = zraw + 4 * idx[r];
        int64_t a = find((int64_t)s[0]), b = find((int64_t)s[1]);
        Z[4 * r + 0] = (double)std::min(a, b);
        Z[4 * r + 1] = (double)std::max(a, b);
        Z[4 * r + 2] = s[2];
        parent[a] = next; parent[b] = next;
        sz[next] = sz[a] + sz[b];
        Z[4 * r + 3] = (double)sz[next];
        next++;
    }
    return HICMI_OK;
}

int hicmi_leaf_order(const double* Z, int64_t n, int32_t* leaves)
{
    if (!Z || !leaves || n < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (n == 1) { leaves[0] = 0; return HICMI_OK; }
    std::vector<int64_t> stack;
    stack.reserve(64);
    stack.push_back(2 * n - 2);
    int64_t out = 0;
    while (!stack.empty()) {
        int64_t node = stack.back(); stack.pop_back();
        if (node < n) { if (out >= n) return fail(HICMI_ESTATE, "malformed linkage"); leaves[out++] = (int32_t)node; continue; }
        const double* row = Z + 4 * (node - n);
        int64_t aa = (int64_t)row[0], ab = (int64_t)row[1];
        int64_t na = aa < n ? 1 : (int64_t)Z[4 * (aa - n) + 3];
        int64_t nb = ab < n ? 1 : (int64_t)Z[4 * (ab - n) + 3];
        // count_sort='ascending': smaller child first; on equal counts keep (Z[i,0], Z[i,1]) order
        if (na > nb) { stack.push_back(aa); stack.push_back(ab); }
        else         { stack.push_back(ab); stack.push_back(aa); }
    }
    return out == n ? HICMI_OK : fail(HICMI_ESTATE, "malformed linkage (%lld leaves of %lld)", (long long)out, (long long)n);
}

// Buffers of the rank matrix: dRank (result), d_order ([order][inverse]), dR (argsort rows of the bitonic path), scratch.
static int ensure_rank_buffers(hicmi_ctx* c, int64_t n, int64_t ldr, bool bitonic)
{
    if (c->r_rows < n || c->ldr != ldr || !c->dRank || !c->d_order) {
        int rc = ensure_all(c->dRank, n * ldr, c->d_order, 2 * n);                      // [order][inverse order]
        if (rc) return rc;
        c->ldr = ldr; c->r_rows = n;
    }
    int rc = bitonic ? ensure(c->dR, n * ldr) : HICMI_OK;
    if (!rc) rc = ensure(c->d_sort_scratch, (int64_t)(bitonic ? sort_scratch_bytes((int)n) : sort_radix_scratch_bytes((int)n)));
    return rc;
}

// The pre-sort.  The nn-chain keeps 8 of the 256 CUs busy for 60 % of Part 1, and the row sort that follows it needs the
// chain's result only for two things: the numbering of rows and columns (the leaf order) and the order of EQUAL
// similarities inside a row.  A row without equal similarities has the same sorted sequence under any numbering, so its
// rank row in leaf labels is the rank row in storage labels re-addressed: rank[a][b] = rank_s[order[a]][order[b]].
// While the chain runs on the main stream, a second low-priority stream therefore sorts every row in storage labels
// (same kernel, identity order, on at most 192 CUs so that the chain's workgroups and its flush kernels always find a
// free one) and notes which rows hold equal keys, and where; hicmi_rank_matrix then only relabels (k_rank_relabel, ~0.5 ms
// at 16k), and finishes the rows with equal keys (sparse maps, fp32 contacts: possibly all of them) with a sort of
// 32-bit (run, leaf position) keys - k_sort_tied.hip.  HICMI_NO_PRESORT=1 disables.
static int start_presort(hicmi_ctx* c, int chain_xcc)
{
    const bool off = getenv("HICMI_NO_PRESORT") != nullptr || getenv("HICMI_SORT_RADIX") != nullptr
                     || getenv("HICMI_SORT_LDS") != nullptr;
    const char* from = getenv("HICMI_PRESORT_FROM");               // (tests lower it; below ~2000 bins the sort is 0.3 ms)
    const int64_t n = c->n;
    c->presort_used = 0;
    if (off || n < (from ? atoll(from) : 2048)) return HICMI_OK;     // (a row shard pre-sorts ALL rows: it is idle meanwhile)
    if (c->presort_n == n) return HICMI_OK;                       // same matrix, same sums: still valid
    const int64_t ldr = (n + 63) & ~(int64_t)63;
    int rc = ensure_rank_buffers(c, n, ldr, true);
    if (rc) return rc;
    if (!c->stream2) {
        int lo = 0, hi = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));         // lo = least urgent
        HIPCHK(hipStreamCreateWithPriority(&c->stream2.h, hipStreamNonBlocking, lo));
    }
    if (!c->ev_fork) {
        HIPCHK(hipEventCreateWithFlags(&c->ev_fork.h, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->ev_join.h, hipEventDisableTiming));
    }
    const int64_t ld_bits = std::max<int64_t>(sort_padded_size((int)n), 16) / 16;
    const bool new_ident = c->d_ident.capacity() < n;             // the identity order is written once per growth
    rc = ensure_all(c->d_ties, 16 + n, c->d_tie_bits, n * ld_bits, c->dRankS, n * ldr, c->d_ident, n);
    if (rc) return rc;
    c->ld_bits = ld_bits;
    if (new_ident) {
        std::vector<int32_t> id((size_t)n);
        for (int64_t i = 0; i < n; i++) id[(size_t)i] = (int32_t)i;
        rc = upload(c, c->d_ident, id.data(), sizeof(int32_t) * (size_t)n);
        if (rc) { c->d_ident.reset(); return rc; }
    }
    HIPCHK(hipEventRecord(c->ev_fork, c->stream));                // sums and identity are in place
    HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
    HIPCHK(hipMemsetAsync(c->d_ties, 0, 16 + (size_t)n, c->stream2));
    {
        Timed t(c, F_PRESORT, (8.0 + 2.0) * (double)n * (double)n, c->stream2);      // N^2 (e + idx) for the row argsort
        SortExtras x;
        x.tie_count = reinterpret_cast<unsigned*>(c->d_ties.get()); x.tie_flag = c->d_ties + 16;
        x.tie_limit = (unsigned)n;                                 // (never gives up: tied rows are finished by k_rank_rows_tied)
        x.tie_bits = c->d_tie_bits; x.ld_bits = ld_bits;
        x.max_workgroups = 192;                                    // (the chain: up to 64 single-wave workgroups, one CU each)
        x.avoid_xcc = chain_xcc;                                   // ... all on one XCD, which this kernel's workgroups leave alone
        x.row_counter = reinterpret_cast<unsigned*>(c->d_ties.get()) + 1;     // (zeroed with the tie count just above)
        if (getenv("HICMI_TEST_PRESORT_ALL_LEAVE")) x.avoid_xcc = -2;      // test hook: every workgroup behaves as if it were on that XCD
        c->presort_dealt = x.avoid_xcc >= 0 || x.avoid_xcc == -2;
        launch_sort_rows(c->dC, c->ldc, c->d_ident, c->d_ident, c->d_np, c->d_seq, (int)n, c->d_sort_scratch, c->dR, ldr, 0, 1,
                         c->stream2, x);
    }
    {
        // (its own family: with the chain's parties holding the LDS of one XCD's CUs, the eighth of this kernel's workgroups
        //  that is dealt to that XCD - 32 KB of LDS each at 16k - waits for the end of a chain epoch; 0.3 ms of work that
        //  can read as 8 ms, all of it beside the chain)
        Timed t(c, F_RANK_INVERT, (2.0 + 2.0) * (double)n * (double)n, c->stream2);
        launch_rank_invert(c->dR, c->dRankS, ldr, (int)n, 0, 1, c->stream2);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev_join, c->stream2));
    c->presort_n = n;
    c->have_rank = false;                                          // dR is being rewritten
    return HICMI_OK;
}

int hicmi_upgma(hicmi_ctx* c, double* Z_out, int32_t* leaves_out)
{
    if (!c || !leaves_out) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    HIPCHK(hipSetDevice(c->device));
    int rc = compute_sums(c);
    if (rc) return rc;
    const int64_t n = c->n;
    if (n == 1) { leaves_out[0] = 0; c->zraw.clear(); return HICMI_OK; }
    const int64_t ldw = (n + 15) & ~(int64_t)15;
    if (c->w_rows < n || c->ldw != ldw || !c->dW) {
        // d_chain: one copy per workgroup of k_nn_epoch_w1 (64) / _mw / _mwc (16)
        rc = ensure_all(c->dW, n * ldw, c->dW2, n * ldw, c->d_size, (int64_t)nnchain_workspace_bytes((int)n),
                        c->d_chain, 64 * (n + 2), c->d_zraw, 4 * n, c->d_status, 1);
        if (rc) return rc;
        c->ldw = ldw; c->w_rows = n;
    }
    static const bool step_prof = getenv("HICMI_STEP_PROFILE") != nullptr;
    std::vector<std::pair<const char*, std::chrono::steady_clock::time_point>> marks;
    auto mark = [&](const char* what) { if (step_prof) marks.emplace_back(what, std::chrono::steady_clock::now()); };
    mark("start");
    {
        Timed t(c, F_BUILD_W, 8.0 * (0.5 * (double)n * (double)n + (double)n * (double)n));
        launch_build_w(c->dC, c->ldc, c->d_np, (int)n, c->dW, ldw, c->stream);
    }
    HIPCHK(hipGetLastError());
    // The pre-sort runs beside the chain on the second stream - from the moment the chain's FIRST cache pass (k_nn_rowmin over
    // the whole matrix, the one full-chip pass the chain has) is queued: started right after k_build_w the pre-sort's 192
    // big workgroups shared the CUs with that pass and stretched it from 0.5 to 2.4 ms at 16k, from 2 to 9.8 ms at 32k.
    const NNChainOptions nn_opt = nnchain_options(c->probed_xcc);
    int presort_rc = HICMI_OK;
    bool presort_started = false;
    auto presort_now = [&] {
        if (!presort_started) { presort_started = true; presort_rc = start_presort(c, nnchain_local_xcc(nn_opt, (int)n)); }
    };
    mark("build_w queued");
    // The nn-chain.  Algorithmic bytes: 8 B x (sum over row scans of the live columns + 3 x sum over merges
    // of the live columns), with the scans counted by the kernels themselves (a scan the neighbour cache answers moves
    // nothing); the merge term is 3 * 8 * sum_{k=0}^{n-2} (n - k).
    struct { int state[16]; unsigned long long prof[8]; unsigned char mail[1152]; unsigned long long detail[32]; } nn;   // the head of the workspace
    for (int attempt = 0; attempt < 3; attempt++) {
        {
            Timed t(c, F_NNCHAIN, 0.0);
            int epochs = launch_nnchain(c->dW, c->dW2, ldw, (int)n, c->d_chain, c->d_zraw, c->d_size, nn_opt, attempt, c->stream,
                                        presort_now);
            presort_now();                                         // (whatever path the chain took)
            if (presort_rc) return presort_rc;
            // the family is reported per epoch launch (the flush / compaction launches in between are ~1 % of it)
            if (epochs > 1) c->launches[F_NNCHAIN] += epochs - 1;
        }
        HIPCHK(hipGetLastError());
        int rc_dl = download(c, &nn, nnchain_state_ptr(c->d_size), sizeof(nn));
        if (rc_dl) return rc_dl;
        c->bytes[F_NNCHAIN] += 8.0 * ((double)nn.prof[5] + 3.0 * (0.5 * (double)(n - 1) * (double)(n + 2)));
        c->nn_scans += (double)nn.prof[6]; c->nn_scan_cols += (double)nn.prof[5]; c->nn_cache_hits += (double)(long long)nn.prof[7];
        c->nn_merges += (double)(n - 1);
        if (nn.state[5] != 2 || attempt > 1) break;
        // A peer workgroup of the column-sliced chain did not answer within its spin budget (a GPU shared with other
        // work can delay a workgroup's start): nothing is wrong with the data.  Rebuild the distances and run the whole
        // chain again - spread over the chip first (had its parties asked for one XCD), then on one workgroup, which
        // waits for nobody.
        fprintf(stderr, "[hicmi] nn-chain: a peer workgroup answered late at merge %d; re-running %s\n", nn.state[0],
                attempt == 0 ? "with the parties spread over the chip" : "on one workgroup");
        c->nn_retries++;
        launch_build_w(c->dC, c->ldc, c->d_np, (int)n, c->dW, ldw, c->stream);
        HIPCHK(hipGetLastError());
    }
    mark("chain (epochs, compactions, state)");
    c->zraw.assign((size_t)(4 * (n - 1)), 0.0);
    {
        int rc_dl = download(c, c->zraw.data(), c->d_zraw, sizeof(double) * 4 * (size_t)(n - 1));
        if (rc_dl) return rc_dl;
    }
    mark("merge records to the host");
    if (nn_opt.profile) {
        const unsigned long long* pr = nn.prof;
        fprintf(stderr, "[hicmi] nnchain phases (ms @100MHz): bookkeeping %.2f scan %.2f pick %.2f merge %.2f update %.2f; "
                        "%llu scans (%.2f per merge), %llu cached steps\n",
                pr[0] / 1e5, pr[1] / 1e5, pr[2] / 1e5, pr[3] / 1e5, pr[4] / 1e5, pr[6], (double)pr[6] / (double)(n - 1), pr[7]);
        const unsigned long long* dq = nn.detail;
        if (dq[0] | dq[2] | dq[3])
            fprintf(stderr, "[hicmi] fused pass detail (ms): issue gathers %.2f, LDS pass %.2f, loads arrive %.2f, compute+stores %.2f, "
                            "gathered+reductions %.2f, stores acked %.2f, barrier %.2f\n",
                    dq[0] / 1e5, dq[1] / 1e5, dq[2] / 1e5, dq[3] / 1e5, dq[4] / 1e5, dq[5] / 1e5, dq[6] / 1e5);
        if (dq[9])
            fprintf(stderr, "[hicmi] one-wave kernel: %llu exchanges, post + polling %.2f ms, %.2f polls of the slowest peer per exchange\n",
                    dq[9], dq[8] / 1e5, (double)dq[10] / (double)dq[9]);
        if (dq[9])
            fprintf(stderr, "[hicmi] stand-alone scans by cause: chain restart %llu, exact tie %llu, neighbour of the merged cluster %llu, "
                            "new neighbour of the row scanned with the merge %llu, reached over cached steps %llu, other %llu\n",
                    dq[12], dq[13], dq[14], dq[15], dq[16], dq[17]);
    }
    if (nn.state[5] == 2)
        return fail(HICMI_ESTATE, "nn-chain: a peer workgroup of the column-sliced kernel answered late, and so did the retry");
    if (nn.state[5] == 3)
        return fail(HICMI_ESTATE, "nn-chain: the replicas of the column-sliced kernel disagree about a merge (stale read between "
                                  "workgroups); set HICMI_NNCHAIN_WGS=1 to run on one workgroup");
    if (nn.state[5] != 0 || nn.state[0] != (int)(n - 1))
        return fail(HICMI_ESTATE, "nn-chain kernel stopped on its guard at merge %d of %lld (NaN distances or an internal error; check %d)",
                    nn.state[0], (long long)(n - 1), nn.state[13]);
    std::vector<double> Z((size_t)(4 * (n - 1)));
    rc = hicmi_label_linkage(c->zraw.data(), n, Z.data());
    if (rc) return rc;
    mark("sort + label");
    rc = hicmi_leaf_order(Z.data(), n, leaves_out);
    if (rc) return rc;
    if (Z_out) memcpy(Z_out, Z.data(), sizeof(double) * Z.size());
    mark("leaf order");
    if (step_prof) {
        fprintf(stderr, "[hicmi] upgma host timeline (ms):");
        for (size_t i = 1; i < marks.size(); i++)
            fprintf(stderr, " %s %.2f%s", marks[i].first, std::chrono::duration<double, std::milli>(marks[i].second - marks[i - 1].second).count(),
                    i + 1 < marks.size() ? "," : "\n");
    }
    return HICMI_OK;
}

int hicmi_get_raw_merges(hicmi_ctx* c, double* out)
{
    if (!c || !out) return fail(HICMI_EINVAL, "bad arguments");
    if (c->zraw.empty()) return fail(HICMI_EINVAL, "hicmi_upgma has not run");
    memcpy(out, c->zraw.data(), sizeof(double) * c->zraw.size());
    return HICMI_OK;
}

int hicmi_nnchain_stats(hicmi_ctx* c, double* out6)
{
    if (!c || !out6) return fail(HICMI_EINVAL, "bad arguments");
    out6[0] = c->nn_merges; out6[1] = c->nn_scans; out6[2] = c->nn_scan_cols; out6[3] = c->nn_cache_hits;
    out6[4] = (double)c->nn_retries; out6[5] = 0.0;
    return HICMI_OK;
}

// ---------------------------------------------------------------------------------------------------
int hicmi_rank_matrix(hicmi_ctx* c, const int32_t* order)
{
    if (!c || !order) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    HIPCHK(hipSetDevice(c->device));
    const int64_t n = c->n;
    static const bool tprof = getenv("HICMI_STEP_PROFILE") != nullptr;
    std::vector<std::chrono::steady_clock::time_point> tm;
    auto tick = [&]() { if (tprof) tm.push_back(std::chrono::steady_clock::now()); };
    auto report = [&]() {
        if (!tprof || tm.size() < 2) return;
        fprintf(stderr, "[hicmi] rank_matrix host timeline (ms):");
        for (size_t i = 1; i < tm.size(); i++) fprintf(stderr, " %.2f", std::chrono::duration<double, std::milli>(tm[i] - tm[i - 1]).count());
        fprintf(stderr, "\n");
    };
    tick();
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; i++) {
        if (order[i] < 0 || order[i] >= n || seen[(size_t)order[i]]) return fail(HICMI_EINVAL, "order is not a permutation of 0..n-1");
        seen[(size_t)order[i]] = 1;
    }
    int rc = compute_sums(c);
    if (rc) return rc;
    const int64_t ldr = (n + 63) & ~(int64_t)63;
    // Default: the register-blocked bitonic network (argsort rows R, then the inversion pass).  HICMI_SORT_RADIX=1: the LSD
    // radix kernel, which writes the rank rows directly - built to get rid of the O(n log^2 n) stages and of the scratch
    // round trips of long rows, verified against the same tests, and measured SLOWER on MI355X (16k / 32k / 64k bins:
    // 15.7 / 87 / 581 ms against 11.7 / 50.6 / 236 ms): 18 passes x 7 workgroup barriers and random 4-byte LDS scatters
    // cost more than the 105 register-resident stages.  Kept as the second implementation the large-map tests compare with.
    const bool bitonic = getenv("HICMI_SORT_RADIX") == nullptr;
    if (c->presort_n != n) c->presort_used = 0;
    tick();
    if (c->presort_n && c->stream2) HIPCHK(hipStreamSynchronize(c->stream2));   // (the buffers below are the pre-sort's too)
    tick();
    rc = ensure_rank_buffers(c, n, ldr, bitonic);
    if (rc) return rc;
    {
        std::vector<int32_t> both((size_t)(2 * n));
        for (int64_t i = 0; i < n; i++) { both[(size_t)i] = order[i]; both[(size_t)(n + order[i])] = (int32_t)i; }
        int rc_up = upload(c, c->d_order, both.data(), sizeof(int32_t) * both.size());
        if (rc_up) return rc_up;
    }
    const double share = 1.0 / (double)c->shard_stride;             // this shard's rows only
    if (c->presort_n == n && bitonic && c->presort_dealt) {
        // The pre-sort's workgroups that were dealt to the chain's XCD left at once and the others took the rows from a
        // counter.  Which workgroup runs where is the hardware's business: had ALL of them landed on that XCD, no row
        // would have been sorted - the counter says how many were handed out.
        unsigned head[4] = {0, 0, 0, 0};
        int rc_dl = download(c, head, c->d_ties, sizeof(head));
        if (rc_dl) return rc_dl;
        if ((int64_t)head[1] < n) {
            fprintf(stderr, "[hicmi] pre-sort: only %u of %lld rows were handed out; sorting now\n", head[1], (long long)n);
            c->presort_n = 0; c->presort_used = 0;
        }
    }
    if (c->presort_n == n && bitonic) {
        // rows sorted in storage labels while the nn-chain ran (start_presort): re-addressed by the leaf order; rows that
        // hold equal keys get the order inside their runs from k_rank_rows_tied
        tick();
        std::vector<unsigned char> ties(16 + (size_t)n);
        int rc_dl = download(c, ties.data(), c->d_ties, ties.size());
        if (rc_dl) return rc_dl;
        tick();
        unsigned n_tied = 0;
        memcpy(&n_tied, ties.data(), sizeof(n_tied));
        // HICMI_PRESORT_TIES=resort: the rows with equal keys go through the full 64-bit sort again (the first version of
        // this path, kept as the A/B for k_rank_rows_tied); it gives the pre-sort up when more than half of the rows do
        const bool resort = getenv("HICMI_PRESORT_TIES") != nullptr && !strcmp(getenv("HICMI_PRESORT_TIES"), "resort");
        c->presort_used = (resort && n_tied > (unsigned)(n / 2)) ? 2 : 1;
        c->presort_tied_rows = (int64_t)n_tied;
        if (c->presort_used == 1) {
            // rows (in leaf numbering) whose storage row holds equal keys: the order inside their runs of equal keys
            // depends on the leaf labels
            std::vector<int32_t> again;                            // (of this shard's rows)
            const int64_t own = (n - c->shard_first + c->shard_stride - 1) / c->shard_stride;
            for (int64_t a = c->shard_first; a < n && n_tied; a += c->shard_stride)
                if (ties[16 + (size_t)order[a]]) again.push_back((int32_t)a);
            if ((int64_t)again.size() < own) {
                Timed t(c, F_RANK_RELABEL, (2.0 + 2.0) * (double)n * (double)(own - (int64_t)again.size()));
                launch_rank_relabel(c->dRankS, c->dRank, ldr, (int)n, c->d_order, (int)c->shard_first, (int)c->shard_stride,
                                    c->stream);
            }
            HIPCHK(hipGetLastError());
            if (!again.empty()) {
                int rc_up = ensure(c->d_row_list, 2 * n);                      // the list + one flag per listed row
                if (!rc_up) rc_up = upload(c, c->d_row_list, again.data(), sizeof(int32_t) * again.size());
                if (rc_up) return rc_up;
                const double part = (double)again.size() / (double)n;
                if (resort) {
                    c->presort_n = 0;                              // dR (the storage-label argsort rows) is overwritten
                    SortExtras x;
                    x.row_list = c->d_row_list; x.n_list = (int)again.size();
                    {
                        Timed t(c, F_SORT, (8.0 + 2.0) * (double)n * (double)n * part);
                        launch_sort_rows(c->dC, c->ldc, c->d_order, c->d_order + n, c->d_np, c->d_seq, (int)n, c->d_sort_scratch,
                                         c->dR, ldr, 0, 1, c->stream, x);
                    }
                    HIPCHK(hipGetLastError());
                    Timed t(c, F_RANK_INVERT, (2.0 + 2.0) * (double)n * (double)n * part);
                    launch_rank_invert(c->dR, c->dRank, ldr, (int)n, 0, 1, c->stream, c->d_row_list, (int)again.size());
                } else {
                    Timed t(c, F_RANK_TIED, (2.0 + 2.0) * (double)n * (double)n * part);
                    launch_rank_rows_tied(c->dR, c->d_tie_bits, c->ld_bits, c->d_order, c->d_order + n, (int)n, c->d_row_list,
                                          (int)again.size(), c->dRank, ldr, c->stream, c->d_row_list + n);
                }
            }
            HIPCHK(hipGetLastError());
            tick();
            HIPCHK(sync_stream(c));
            tick();
            report();
            c->have_rank = true;
            c->cached_start = -1;
            return HICMI_OK;
        }
    }
    c->presort_n = 0;                                               // (dR is overwritten below)
    if (!bitonic) {
        Timed t(c, F_SORT, (8.0 + 2.0) * (double)n * (double)n * share);
        launch_rank_rows_radix(c->dC, c->ldc, c->d_order, c->d_order + n, c->d_np, c->d_seq, (int)n, c->d_sort_scratch, c->dRank,
                               ldr, (int)c->shard_first, (int)c->shard_stride, c->stream);
    } else {
        {
            Timed t(c, F_SORT, (8.0 + 2.0) * (double)n * (double)n * share);
            launch_sort_rows(c->dC, c->ldc, c->d_order, c->d_order + n, c->d_np, c->d_seq, (int)n, c->d_sort_scratch, c->dR, ldr,
                             (int)c->shard_first, (int)c->shard_stride, c->stream);
        }
        HIPCHK(hipGetLastError());
        Timed t(c, F_RANK_INVERT, (2.0 + 2.0) * (double)n * (double)n * share);
        launch_rank_invert(c->dR, c->dRank, ldr, (int)n, (int)c->shard_first, (int)c->shard_stride, c->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(sync_stream(c));
    c->have_rank = true;
    c->cached_start = -1;
    return HICMI_OK;
}

int hicmi_presort_state(hicmi_ctx* c, int* state_out, int64_t* tied_rows_out)
{
    if (!c || !state_out) return fail(HICMI_EINVAL, "bad arguments");
    *state_out = c->presort_used;
    if (tied_rows_out) *tied_rows_out = c->presort_used ? c->presort_tied_rows : 0;
    return HICMI_OK;
}

int hicmi_get_rank_rows(hicmi_ctx* c, int64_t row0, int64_t nrows, int inverse, uint16_t* out)
{
    if (!c || !out || row0 < 0 || nrows < 0) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->have_rank) return fail(HICMI_EINVAL, "hicmi_rank_matrix has not run");
    if (row0 + nrows > c->n) return fail(HICMI_EINVAL, "rows out of range");
    HIPCHK(hipSetDevice(c->device));
    // the device keeps the RANK rows (position of every column); an argsort row is their inverse, formed here on request
    const uint16_t* src = c->dRank + row0 * c->ldr;
    HIPCHK(hipMemcpy2DAsync(out, sizeof(uint16_t) * (size_t)c->n, src, sizeof(uint16_t) * (size_t)c->ldr,
                            sizeof(uint16_t) * (size_t)c->n, (size_t)nrows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_stream(c));
    if (!inverse) {
        std::vector<uint16_t> tmp((size_t)c->n);
        for (int64_t r = 0; r < nrows; r++) {
            uint16_t* row = out + r * c->n;
            for (int64_t col = 0; col < c->n; col++) {
                if (row[col] >= c->n) return fail(HICMI_ESTATE, "rank row %lld is not a permutation (a row of another shard?)", (long long)(row0 + r));
                tmp[row[col]] = (uint16_t)col;
            }
            memcpy(row, tmp.data(), sizeof(uint16_t) * (size_t)c->n);
        }
    }
    return HICMI_OK;
}

int hicmi_get_similarity_row(hicmi_ctx* c, int64_t row, double* out)
{
    if (!c || !out) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->have_rank) return fail(HICMI_EINVAL, "hicmi_rank_matrix has not run");
    if (row < 0 || row >= c->n) return fail(HICMI_EINVAL, "row out of range");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure(c->d_tmp, c->n);
    if (rc) return rc;
    launch_similarity_row(c->dC, c->ldc, c->d_order, c->d_np, c->d_seq, (int)c->n, (int)row, c->d_tmp, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->d_tmp, sizeof(double) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

// ---------------------------------------------------------------------------------------------------
static int ensure_scan_buffers(hicmi_ctx* c)
{
    return ensure_all(c->d_x, c->n, c->d_sig, c->n);
}

// The significance flags of the rows counted in d_x.  The flags are all the host loops need, tens of thousands of
// times per map: the kernel writes them straight into the pinned buffer (no copy kernel, one synchronisation).
static int finish_scan(hicmi_ctx* c, int64_t rows, int mode, int64_t L_fixed, int64_t M, double psig, int32_t* x_out,
                       uint8_t* sig_out, int64_t own_first)
{
    const bool direct = sig_out && !x_out;
    if (direct) { int rc = ensure_pin_down(c, (size_t)rows); if (rc) return rc; }
    {
        Timed t(c, F_HYPER_FLAGS, 5.0 * (double)rows);
        launch_hyper_flags(c->d_x, (int)rows, mode, (int)L_fixed, M, psig, direct ? reinterpret_cast<uint8_t*>(c->pin_down.get()) : c->d_sig,
                           (int)own_first, (int)c->shard_stride, c->stream);
    }
    HIPCHK(hipGetLastError());
    if (direct) {
        HIPCHK(sync_stream(c));
        memcpy(sig_out, c->pin_down, (size_t)rows);
        return HICMI_OK;
    }
    if (x_out) { int rc = download(c, x_out, c->d_x, sizeof(int32_t) * (size_t)rows); if (rc) return rc; }
    if (sig_out) { int rc = download(c, sig_out, c->d_sig, (size_t)rows); if (rc) return rc; }
    if (!x_out && !sig_out) HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_cut_scan(hicmi_ctx* c, int64_t start, int64_t M, double psig, int32_t* x_out, uint8_t* sig_out)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (!c->have_rank) return fail(HICMI_EINVAL, "hicmi_rank_matrix has not run");
    const int64_t n = c->n;
    if (start < 0 || start >= n) return fail(HICMI_EINVAL, "start out of range");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_scan_buffers(c);
    if (rc) return rc;
    const int64_t cnt = n - start;              // entries: rows start .. n-1
    const int64_t st = c->shard_stride;
    const int64_t t0 = ((c->shard_first - start) % st + st) % st;      // first entry whose row this shard owns
    if (c->cached_start != start) {
        HIPCHK(hipMemsetAsync(c->d_x, 0, sizeof(int32_t) * (size_t)(st > 1 ? cnt : 1), c->stream));
        const double m = (double)(cnt - 1);
        Timed t(c, F_CUT_COUNT, 2.0 * (m * (m + 3.0) / 2.0) / (double)st);      // sum_{L=1..m} (L+1) uint16 entries
        const int64_t t1 = t0 >= 1 ? t0 : t0 + st;                      // entry 0 (the row `start` itself) is never counted
        if (t1 < cnt)
            launch_cut_count(c->dRank, c->ldr, (int)(start + t1), (int)(cnt - t1), (int)start, 0, 0, c->d_x + t1, (int)st, c->stream);
        HIPCHK(hipGetLastError());
        c->cached_start = start;
    }
    return finish_scan(c, cnt, 0, 0, M, psig, x_out, sig_out, t0);
}

int hicmi_filter_scan(hicmi_ctx* c, int64_t start, int64_t cut, int64_t n_rows, int64_t M, double psig,
                      int32_t* x_out, uint8_t* sig_out)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (!c->have_rank) return fail(HICMI_EINVAL, "hicmi_rank_matrix has not run");
    const int64_t n = c->n;
    if (start < 0 || start >= n || cut < start || cut >= n || n_rows < 0 || start + n_rows > n)
        return fail(HICMI_EINVAL, "filter scan arguments out of range");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_scan_buffers(c);
    if (rc) return rc;
    c->cached_start = -1;                       // d_x is reused
    const int64_t st = c->shard_stride;
    const int64_t t0 = ((c->shard_first - start) % st + st) % st;      // first entry whose row this shard owns
    if (st > 1) HIPCHK(hipMemsetAsync(c->d_x, 0, sizeof(int32_t) * (size_t)n_rows, c->stream));
    {
        Timed t(c, F_CUT_COUNT, 2.0 * (double)n_rows * (double)(cut - start + 1) / (double)st);
        if (t0 < n_rows)
            launch_cut_count(c->dRank, c->ldr, (int)(start + t0), (int)(n_rows - t0), (int)start, 1, (int)cut, c->d_x + t0, (int)st,
                             c->stream);
    }
    HIPCHK(hipGetLastError());
    return finish_scan(c, n_rows, 1, cut - start, M, psig, x_out, sig_out, t0);
}

double hicmi_hypergeom_sf(int64_t x, int64_t M, int64_t n, int64_t N) { return hypergeom_sf_ge(x, M, n, N); }
int hicmi_hypergeom_decide(int64_t x, int64_t M, int64_t n, int64_t N, double psig) { return hypergeom_decide(x, M, n, N, psig); }

// ---- the two scan loops with their control flow on the device (k_part1_scan.hip) -------------------------------------
// Up to SCAN_MAX_SETS parameter sets in lock step; the single-set entries are the one-set case.  One allocation, sized
// from n_sets x n: [ScanState x SCAN_MAX_SETS], then per set x n, cuts n, M log 2n, alt n, seg 3n, seg_x n int32 and
// sig n, filt n, prev n bytes (39 B per row and set).
static_assert(SCAN_MAX_SETS == HICMI_SCAN_MAX_SETS, "hicmi.h and the kernels disagree on the set cap");

struct ScanMulti {
    ScanState* st; int32_t *x, *cuts, *mlog, *alt, *seg, *seg_x; uint8_t *sig, *filt, *prev;
};

static int ensure_scan_multi(hicmi_ctx* c, int sets, ScanMulti& m)
{
    const size_t n = (size_t)c->n, S = (size_t)sets;
    const size_t head = (sizeof(ScanState) * SCAN_MAX_SETS + 255) & ~(size_t)255;
    const size_t bytes = head + S * n * (sizeof(int32_t) * 9 + 3) + 64;
    int rc = ensure(c->d_scan_multi, (int64_t)bytes);
    if (rc) return rc;
    unsigned char* b = c->d_scan_multi;
    m.st = reinterpret_cast<ScanState*>(b);
    m.x = reinterpret_cast<int32_t*>(b + head);
    m.cuts = m.x + S * n; m.mlog = m.cuts + S * n; m.alt = m.mlog + 2 * S * n; m.seg = m.alt + S * n; m.seg_x = m.seg + 3 * S * n;
    m.sig = reinterpret_cast<uint8_t*>(m.seg_x + S * n); m.filt = m.sig + S * n; m.prev = m.filt + S * n;
    return HICMI_OK;
}

static int scan_share()
{
    const char* e = getenv("HICMI_SCAN_SHARE");                    // "0": every set counts its own rows (the A/B)
    return e && !strcmp(e, "0") ? 0 : 1;
}

// Batches of lock-step scans until every set's loop has ended.  `pairs` launches per batch: the records are read once
// per batch, and the runaway guard applies to every set on its own.
static int run_scan_multi(hicmi_ctx* c, std::vector<ScanState>& h, const ScanMulti& m, const std::vector<int64_t>& max_scans,
                          const std::function<void(int)>& enqueue)
{
    const size_t S = h.size();
    int rc = upload(c, m.st, h.data(), sizeof(ScanState) * S);
    if (rc) return rc;
    const int pairs = 32;
    int64_t batches = 0;
    for (int64_t issued = 0; ; issued += pairs) {
        bool all_done = true;
        for (size_t k = 0; k < S; k++) {
            if (h[k].done) continue;
            all_done = false;
            if (issued > max_scans[k] + pairs)
                return fail(HICMI_ESTATE, "scan loop of set %d did not end after %lld scans", (int)k, (long long)issued);
        }
        if (all_done) break;
        {
            Timed t(c, F_CUT_COUNT, 0.0);
            enqueue(pairs);
        }
        HIPCHK(hipGetLastError());
        batches++;
        rc = download(c, h.data(), m.st, sizeof(ScanState) * S);
        if (rc) return rc;
    }
    int64_t scans = 0; double bytes = 0;
    for (const ScanState& r : h) { scans += r.scans; bytes += (double)r.bytes; }
    // the family is reported per set and scan; the flags are decided inside k_cut_rows, by the lanes that hold the counts: no
    // launch of the hyper_flags family, which is k_hyper_flags after a scan driven from the host (finish_scan)
    c->launches[F_CUT_COUNT] += scans - batches;
    c->bytes[F_CUT_COUNT] += bytes;
    return HICMI_OK;
}

// A first-pass set's record before its first scan.
static ScanState first_pass_record(int64_t n, int64_t min_size, int64_t stop_ind, double psig)
{
    ScanState r;
    memset(&r, 0, sizeof(r));
    r.mode = 0; r.start = 0; r.M = n; r.recount = 1; r.psig = psig;
    r.min_size = (int)std::min<int64_t>(min_size, n + 1); r.stop_ind = (int)std::min<int64_t>(stop_ind, INT32_MAX);
    return r;
}

// A filter set's record before its first scan: n_in candidates, the first of them `first`.
static ScanState filter_record(int64_t n, int64_t n_in, int32_t first, double psig)
{
    ScanState r;
    memset(&r, 0, sizeof(r));
    r.mode = 1; r.start = 0; r.M = n; r.recount = 1; r.psig = psig;
    r.MD = (int)(n / 5);                                           // MD = int(n / 5)  (S2C:575)
    r.n_alt = (int)n_in; r.f_max_rounds = (int)std::min<int64_t>(10 * n_in, INT32_MAX);   // S2C:577
    r.cut = first;
    r.n_rows = (int)std::min<int64_t>(n, (int64_t)r.MD + 1);
    r.done = n_in == 0;                                            // nothing to filter
    return r;
}

int hicmi_first_pass_cuts(hicmi_ctx* c, int64_t min_size, int64_t stop_ind, double psig, int32_t* cuts_out, int64_t cuts_cap,
                          int64_t* n_cuts_out, int32_t* m_log_out, int64_t log_cap, int64_t* n_log_out)
{
    return hicmi_first_pass_cuts_multi(c, 1, &min_size, &stop_ind, psig, cuts_out, cuts_cap, n_cuts_out, m_log_out, log_cap,
                                       n_log_out);
}

int hicmi_filter_cuts(hicmi_ctx* c, const int32_t* cuts_in, int64_t n_in, double psig, int32_t* cuts_out, int64_t cuts_cap,
                      int64_t* n_out, int64_t* warned_out)
{
    if (!c || !cuts_in || !cuts_out || !n_out || n_in < 1) return fail(HICMI_EINVAL, "bad arguments");
    const int64_t cand_off[2] = {0, n_in};
    int64_t warned = 0;
    const int rc = hicmi_filter_cuts_multi(c, 1, cand_off, cuts_in, &psig, cuts_out, cuts_cap, n_out, &warned);
    if (!rc && warned_out) *warned_out = warned;
    return rc;
}

int hicmi_first_pass_cuts_multi(hicmi_ctx* c, int64_t n_sets, const int64_t* min_size, const int64_t* stop_ind, double psig,
                                int32_t* cuts_out, int64_t cuts_cap, int64_t* n_cuts_out, int32_t* m_log_out, int64_t log_cap,
                                int64_t* n_log_out)
{
    if (!c || !min_size || !stop_ind || !cuts_out || !n_cuts_out || !n_log_out || (log_cap > 0 && !m_log_out))
        return fail(HICMI_EINVAL, "bad arguments");
    if (n_sets < 1 || n_sets > SCAN_MAX_SETS) return fail(HICMI_EINVAL, "n_sets must be in [1, %d]", SCAN_MAX_SETS);
    if (!c->have_rank) return fail(HICMI_EINVAL, "hicmi_rank_matrix has not run");
    if (c->shard_stride != 1) return fail(HICMI_EINVAL, "the device-driven scan loops need the whole rank matrix (no row shard)");
    for (int64_t k = 0; k < n_sets; k++)
        if (min_size[k] < 1) return fail(HICMI_EINVAL, "min_size must be >= 1 (set %lld)", (long long)k);
    const int64_t n = c->n;
    HIPCHK(hipSetDevice(c->device));
    ScanMulti m;
    int rc = ensure_scan_multi(c, (int)n_sets, m);
    if (rc) return rc;
    std::vector<ScanState> h((size_t)n_sets);
    for (int64_t k = 0; k < n_sets; k++) h[(size_t)k] = first_pass_record(n, min_size[k], stop_ind[k], psig);
    const int lcap = (int)n;                                       // pairs that fit the device log
    const int share = scan_share();
    rc = run_scan_multi(c, h, m, std::vector<int64_t>((size_t)n_sets, 6 * n), [&](int pairs) {
        launch_first_pass_multi_pairs(c->dRank, c->ldr, (int)n, (int)n_sets, m.st, m.x, m.sig, psig, share, m.cuts, m.mlog,
                                      lcap, pairs, c->stream);
    });
    if (rc) return rc;
    for (int64_t k = 0; k < n_sets; k++) {
        const ScanState& r = h[(size_t)k];
        if (r.n_cuts > cuts_cap) return fail(HICMI_EINVAL, "%d cuts of set %lld do not fit cuts_cap", r.n_cuts, (long long)k);
        if (r.n_log > lcap || r.n_log > log_cap) return fail(HICMI_EINVAL, "%d M changes of set %lld do not fit the log", r.n_log, (long long)k);
    }
    for (int64_t k = 0; k < n_sets; k++) {
        const ScanState& r = h[(size_t)k];
        if (r.n_cuts) { rc = download(c, cuts_out + k * cuts_cap, m.cuts + k * n, sizeof(int32_t) * (size_t)r.n_cuts); if (rc) return rc; }
        if (r.n_log) { rc = download(c, m_log_out + 2 * k * log_cap, m.mlog + 2 * k * n, sizeof(int32_t) * 2 * (size_t)r.n_log); if (rc) return rc; }
        n_cuts_out[k] = r.n_cuts; n_log_out[k] = r.n_log;
    }
    return HICMI_OK;
}

int hicmi_filter_cuts_multi(hicmi_ctx* c, int64_t n_sets, const int64_t* cand_off, const int32_t* cuts_in, const double* psig,
                            int32_t* cuts_out, int64_t cuts_cap, int64_t* n_out, int64_t* warned_out)
{
    if (!c || !cand_off || !psig || !cuts_out || !n_out || !warned_out) return fail(HICMI_EINVAL, "bad arguments");
    if (n_sets < 1 || n_sets > SCAN_MAX_SETS) return fail(HICMI_EINVAL, "n_sets must be in [1, %d]", SCAN_MAX_SETS);
    if (!c->have_rank) return fail(HICMI_EINVAL, "hicmi_rank_matrix has not run");
    if (c->shard_stride != 1) return fail(HICMI_EINVAL, "the device-driven scan loops need the whole rank matrix (no row shard)");
    const int64_t n = c->n;
    if (cand_off[0] != 0) return fail(HICMI_EINVAL, "cand_off[0] must be 0");
    for (int64_t k = 0; k < n_sets; k++) {
        const int64_t a = cand_off[k], b = cand_off[k + 1];
        if (b < a || b - a > n) return fail(HICMI_EINVAL, "candidate list %lld: bad offsets", (long long)k);
        if (b > a && !cuts_in) return fail(HICMI_EINVAL, "bad arguments");
        for (int64_t i = a; i < b; i++)
            if (cuts_in[i] < 0 || cuts_in[i] >= n || (i > a && cuts_in[i] <= cuts_in[i - 1]))
                return fail(HICMI_EINVAL, "cuts must be ascending indices in [0, n) (set %lld)", (long long)k);
    }
    HIPCHK(hipSetDevice(c->device));
    ScanMulti m;
    int rc = ensure_scan_multi(c, (int)n_sets, m);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(m.filt, 0, 2 * (size_t)n_sets * (size_t)n, c->stream));   // filtered = {}, prev_filtered = {}
    std::vector<ScanState> h((size_t)n_sets);
    std::vector<int64_t> max_scans((size_t)n_sets);
    const int max_rows = (int)std::min<int64_t>(n, n / 5 + 1);
    for (int64_t k = 0; k < n_sets; k++) {
        const int64_t a = cand_off[k], n_in = cand_off[k + 1] - a;
        h[(size_t)k] = filter_record(n, n_in, n_in ? cuts_in[a] : 0, psig[k]);
        // every pass over the candidates runs at most 10 * n_in rounds of at most n_in scans; the passes end when the
        // set of kept cuts repeats - bounded here far above anything a map produces
        max_scans[(size_t)k] = std::min<int64_t>((int64_t)4000000, 20 * n_in * n_in * 10 + 1000);
        if (n_in) { rc = upload(c, m.alt + k * n, cuts_in + a, sizeof(int32_t) * (size_t)n_in); if (rc) return rc; }
    }
    const int share = scan_share();
    rc = run_scan_multi(c, h, m, max_scans, [&](int pairs) {
        launch_filter_multi_pairs(c->dRank, c->ldr, (int)n, max_rows, (int)n_sets, m.st, m.x, m.sig, psig[0], share, m.alt,
                                  m.filt, m.prev, m.seg, m.seg_x, pairs, c->stream);
    });
    if (rc) return rc;
    std::vector<uint8_t> kept((size_t)n_sets * (size_t)n);
    rc = download(c, kept.data(), m.filt, kept.size());
    if (rc) return rc;
    for (int64_t k = 0; k < n_sets; k++) {
        int64_t cnt = 0;
        const uint8_t* f = kept.data() + (size_t)k * (size_t)n;
        for (int64_t e = 0; e < n; e++)
            if (f[e]) {
                if (cnt >= cuts_cap) return fail(HICMI_EINVAL, "filtered cuts of set %lld do not fit cuts_cap", (long long)k);
                cuts_out[k * cuts_cap + cnt++] = (int32_t)e;
            }
        n_out[k] = cnt;
        warned_out[k] = h[(size_t)k].f_warned;
    }
    return HICMI_OK;
}

// ---------------------------------------------------------------------------------------------------
namespace {
// H[k] = 1 + 1/2 + ... + 1/k, left to right in fp64 (H[0] = 0): entries [0, n]
void harmonic_table(std::vector<double>& H, int64_t n)
{
    H.assign((size_t)(n + 1), 0.0);
    for (int64_t k = 1; k <= n; k++) H[(size_t)k] = H[(size_t)k - 1] + 1.0 / (double)k;
}

// hicmi_p2_select without its wait: the H table (when it has to grow; `H_shared`, if given, holds at least n + 1 entries of
// harmonic_table), the selection and the gather kernel are queued on the context's stream
int select_enqueue(hicmi_ctx* c, const int32_t* sel, int64_t n, const std::vector<double>* H_shared)
{
    if (!c || !sel || n < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    for (int64_t i = 0; i < n; i++)
        if (sel[i] < 0 || sel[i] >= c->n) return fail(HICMI_EINVAL, "selection index out of range");
    HIPCHK(hipSetDevice(c->device));
    const int64_t ld2 = (n + 15) & ~(int64_t)15;
    int rc = ensure(c->dM2, n * ld2);
    if (!rc) rc = ensure(c->d_sel, n);
    if (rc) return rc;
    if (c->d_H.capacity() < n + 1) {
        std::vector<double> own;
        if (!H_shared || (int64_t)H_shared->size() < n + 1) { harmonic_table(own, n); H_shared = &own; }
        rc = ensure(c->d_H, n + 1);
        if (rc) return rc;
        rc = upload(c, c->d_H, H_shared->data(), sizeof(double) * (size_t)(n + 1));
        if (rc) { c->d_H.reset(); return rc; }                    // (a table that was not written is not kept)
    }
    rc = upload(c, c->d_sel, sel, sizeof(int32_t) * (size_t)n);
    if (rc) return rc;
    {
        Timed t(c, F_P2_SELECT, 16.0 * (double)n * (double)n);
        launch_p2_select(c->dC, c->ldc, c->d_sel, (int)n, c->dM2, ld2, c->stream);
    }
    HIPCHK(hipGetLastError());
    c->n2 = n; c->ld2 = ld2;
    c->n_scaf = 0; c->n_arr = 0; c->h_arr_id.clear();
    c->cache_valid = false; c->exact_cache.clear();
    return HICMI_OK;
}
}  // namespace

int hicmi_p2_select(hicmi_ctx* c, const int32_t* sel, int64_t n)
{
    int rc = select_enqueue(c, sel, n, nullptr);
    if (rc) return rc;
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_p2_total(hicmi_ctx* c, double* total_out)
{
    if (!c || !total_out) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n2 < 1) return fail(HICMI_EINVAL, "hicmi_p2_select has not run");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure(c->d_partial, c->n2 + 1);
    if (rc) return rc;
    {
        Timed t(c, F_P2_TOTAL, 4.0 * (double)c->n2 * (double)c->n2);
        launch_p2_total(c->dM2, c->ld2, (int)c->n2, c->d_partial, c->d_partial + c->n2, c->stream);
    }
    HIPCHK(hipGetLastError());
    return download(c, total_out, c->d_partial + c->n2, sizeof(double));
}

int hicmi_p2_score(hicmi_ctx* c, const int32_t* perms, int64_t n_cand, int64_t n_used, double total, double* scores_out)
{
    if (!c || !perms || !scores_out || n_cand < 0 || n_used < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n2 < 1) return fail(HICMI_EINVAL, "hicmi_p2_select has not run");
    if (n_used > c->n2) return fail(HICMI_EINVAL, "n_used exceeds the selection");
    if (n_cand == 0) return HICMI_OK;
    if (int rc = check_candidate_bins(n_used)) return rc;
    for (int64_t i = 0; i < n_cand * n_used; i++)
        if (perms[i] < 0 || perms[i] >= c->n2) return fail(HICMI_EINVAL, "candidate index out of range");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure(c->d_perms, n_cand * n_used);
    if (!rc) rc = ensure(c->d_scores, n_cand);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->d_perms, perms, sizeof(int32_t) * (size_t)(n_cand * n_used), hipMemcpyHostToDevice, c->stream));
    {
        Timed t(c, F_P2_SCORE, 8.0 * (double)n_cand * 0.5 * (double)n_used * (double)(n_used - 1));
        launch_p2_score(c->dM2, c->ld2, c->d_perms, (int)n_cand, (int)n_used, c->d_H, 0.0, total, c->d_scores, c->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(scores_out, c->d_scores, sizeof(double) * (size_t)n_cand, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_p2_score_exact(hicmi_ctx* c, const int32_t* perms, int64_t n_cand, int64_t n_used, double total,
                         double* scores_out)
{
    if (!c || !perms || !scores_out || n_cand < 0 || n_used < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n2 < 1) return fail(HICMI_EINVAL, "hicmi_p2_select has not run");
    if (n_used > c->n2) return fail(HICMI_EINVAL, "n_used exceeds the selection");
    if (n_cand == 0) return HICMI_OK;
    if (int rc = check_candidate_bins(n_used)) return rc;
    for (int64_t i = 0; i < n_cand * n_used; i++)
        if (perms[i] < 0 || perms[i] >= c->n2) return fail(HICMI_EINVAL, "candidate index out of range");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure(c->d_perms, n_cand * n_used);
    if (!rc) rc = ensure(c->d_scores, n_cand);
    if (!rc) rc = ensure(c->d_T, 2 * n_cand * n_used);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->d_perms, perms, sizeof(int32_t) * (size_t)(n_cand * n_used), hipMemcpyHostToDevice, c->stream));
    {
        Timed t(c, F_P2_EXACT, 8.0 * (double)n_cand * 0.5 * (double)n_used * (double)(n_used - 1));
        launch_p2_score_exact(c->dM2, c->ld2, c->d_perms, (int)n_cand, (int)n_used, total, c->d_T,
                              c->d_T + n_cand * n_used, c->d_scores, c->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(scores_out, c->d_scores, sizeof(double) * (size_t)n_cand, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}


// ---------------------------------------------------------------------------------------------------
// Part 2 search with device-side candidate enumeration (k_part2_search.hip)
int hicmi_p2_layout(hicmi_ctx* c, const int32_t* scaf_start, const int32_t* scaf_len, int64_t n_scaf)
{
    if (!c || !scaf_start || !scaf_len || n_scaf < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n2 < 1) return fail(HICMI_EINVAL, "hicmi_p2_select has not run");
    for (int64_t i = 0; i < n_scaf; i++)
        if (scaf_len[i] < 1 || scaf_start[i] < 0 || (int64_t)scaf_start[i] + scaf_len[i] > c->n2)
            return fail(HICMI_EINVAL, "scaffold %lld is not a range of the selection", (long long)i);
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_all(c->d_scaf_start, n_scaf, c->d_scaf_len, n_scaf);
    if (rc) return rc;
    c->h_scaf_start.assign(scaf_start, scaf_start + n_scaf);
    c->h_scaf_len.assign(scaf_len, scaf_len + n_scaf);
    c->n_scaf = n_scaf; c->n_arr = 0;
    int rc_up = upload(c, c->d_scaf_start, scaf_start, sizeof(int32_t) * (size_t)n_scaf);
    if (rc_up) return rc_up;
    return upload(c, c->d_scaf_len, scaf_len, sizeof(int32_t) * (size_t)n_scaf);     // consumed in stream order
}

int hicmi_p2_set_arrangement(hicmi_ctx* c, const int32_t* ids, const uint8_t* rev, int64_t S)
{
    if (!c || !ids || !rev || S < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n_scaf < 1) return fail(HICMI_EINVAL, "hicmi_p2_layout has not run");
    std::vector<int32_t> pos((size_t)S + 1, 0);
    std::vector<uint8_t> used((size_t)c->n_scaf, 0);
    for (int64_t j = 0; j < S; j++) {
        if (ids[j] < 0 || ids[j] >= c->n_scaf || used[(size_t)ids[j]]) return fail(HICMI_EINVAL, "arrangement must list distinct scaffolds of the layout");
        used[(size_t)ids[j]] = 1;
        pos[(size_t)j + 1] = pos[(size_t)j] + c->h_scaf_len[(size_t)ids[j]];
    }
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure(c->d_arr_packed, 3 * std::max<int64_t>(S, c->n_scaf) + 2);
    if (!rc) rc = ensure(c->d_pos2sel, c->n2);
    if (rc) return rc;
    c->h_arr_id.assign(ids, ids + S); c->h_arr_rev.assign(rev, rev + S); c->h_arr_pos = pos;
    c->arr_version++;
    c->n_arr = pos[(size_t)S];
    c->h_pos2sel.resize((size_t)c->n_arr);
    for (int64_t j = 0; j < S; j++) {
        const int32_t st = c->h_scaf_start[(size_t)ids[j]], ln = c->h_scaf_len[(size_t)ids[j]];
        int32_t* dst = c->h_pos2sel.data() + pos[(size_t)j];
        if (rev[j]) for (int32_t e = 0; e < ln; e++) dst[e] = st + ln - 1 - e;
        else        for (int32_t e = 0; e < ln; e++) dst[e] = st + e;
    }
    c->h_arr_packed.resize((size_t)(3 * S + 1));
    for (int64_t j = 0; j < S; j++) { c->h_arr_packed[(size_t)j] = ids[j]; c->h_arr_packed[(size_t)(2 * S + 1 + j)] = rev[j] ? 1 : 0; }
    for (int64_t j = 0; j <= S; j++) c->h_arr_packed[(size_t)(S + j)] = pos[(size_t)j];
    rc = upload(c, c->d_arr_packed, c->h_arr_packed.data(), sizeof(int32_t) * (size_t)(3 * S + 1));
    if (rc) return rc;
    launch_arr_materialize(c->d_arr_packed, (int)S, c->d_scaf_start, c->d_scaf_len, (int)c->n_arr, c->d_pos2sel, c->stream);
    HIPCHK(hipGetLastError());
    return HICMI_OK;
}

namespace {
// hicmi_p2_arrangement_total without its wait: the kernel and the copy of the total to the head of the pinned download
// buffer are queued; the value is there after sync_stream
int arrangement_total_enqueue(hicmi_ctx* c)
{
    if (c->n_arr < 1) return fail(HICMI_EINVAL, "hicmi_p2_set_arrangement has not run");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure(c->d_T, c->n_arr + 1);
    if (!rc) rc = ensure(c->d_scores, 1);
    if (rc) return rc;
    rc = ensure_pin_down(c, sizeof(double));
    if (rc) return rc;
    {
        Timed t(c, F_P2_TOTAL, 4.0 * (double)c->n_arr * (double)c->n_arr);
        launch_p2_total_perm(c->dM2, c->ld2, c->d_pos2sel, (int)c->n_arr, c->d_T, c->d_scores, c->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->pin_down, c->d_scores, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return HICMI_OK;
}
}  // namespace

int hicmi_p2_arrangement_total(hicmi_ctx* c, double* total_out)
{
    if (!c || !total_out) return fail(HICMI_EINVAL, "bad arguments");
    int rc = arrangement_total_enqueue(c);
    if (rc) return rc;
    HIPCHK(sync_stream(c));
    memcpy(total_out, c->pin_down, sizeof(double));
    return HICMI_OK;
}

int hicmi_p2_arrangement_score(hicmi_ctx* c, double total, double* score_out)
{
    if (!c || !score_out) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n_arr < 1) return fail(HICMI_EINVAL, "hicmi_p2_set_arrangement has not run");
    if (c->n_arr < 2) { *score_out = 0.0; return HICMI_OK; }
    HIPCHK(hipSetDevice(c->device));
    const int NB = kBaseSlabs;
    int rc = ensure(c->d_scores, NB);
    if (rc) return rc;
    {
        Timed t(c, F_P2_SCORE, 4.0 * (double)c->n_arr * (double)(c->n_arr - 1));
        launch_p2_base_partial(c->dM2, c->ld2, c->d_pos2sel, (int)c->n_arr, c->d_H, (int)c->n_arr, NB, c->d_scores, c->stream);
    }
    HIPCHK(hipGetLastError());
    double part[NB];
    rc = download(c, part, c->d_scores, sizeof(double) * NB);
    if (rc) return rc;
    double sum = 0.0;
    for (int b = 0; b < NB; b++) sum += part[b];
    *score_out = sum / total;
    return HICMI_OK;
}

int hicmi_p2_score_insertions(hicmi_ctx* c, int32_t new_id, double total, double* scores_out)
{
    if (!c || !scores_out) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n_scaf < 1) return fail(HICMI_EINVAL, "hicmi_p2_layout has not run");
    if (new_id < 0 || new_id >= c->n_scaf) return fail(HICMI_EINVAL, "new scaffold out of range");
    const int64_t S = (int64_t)c->h_arr_id.size();
    if (c->n_arr < 1 || S < 1) return fail(HICMI_EINVAL, "hicmi_p2_set_arrangement has not run");
    for (int64_t j = 0; j < S; j++) if (c->h_arr_id[(size_t)j] == new_id) return fail(HICMI_EINVAL, "scaffold is already in the arrangement");
    const int new_len = c->h_scaf_len[(size_t)new_id];
    if (int rc = check_candidate_bins(c->n_arr + new_len)) return rc;
    HIPCHK(hipSetDevice(c->device));
    // incremental form: BASE (64 partial sums) - STRADDLE(g) (prefix sums of S increments) + CROSS(g, r)
    const int NB = kBaseSlabs;
    const int64_t n_out = NB + S + 2 * (S + 1);
    int rc = ensure(c->d_scores, n_out);
    if (rc) return rc;
    {
        const double nn = (double)c->n_arr;
        Timed t(c, F_P2_INSERT, 8.0 * (0.5 * nn * (nn - 1.0) + nn * nn + 2.0 * (double)(S + 1) * (double)new_len * nn));
        launch_p2_insert_delta(c->dM2, c->ld2, c->d_pos2sel, (int)c->n_arr, c->d_arr_packed + S, (int)S,
                               c->h_scaf_start[(size_t)new_id], new_len, c->d_H, NB, c->d_scores, c->stream);
    }
    HIPCHK(hipGetLastError());
    std::vector<double> host((size_t)n_out);
    rc = download(c, host.data(), c->d_scores, sizeof(double) * (size_t)n_out);
    if (rc) return rc;
    double base = 0.0;
    for (int b = 0; b < NB; b++) base += host[(size_t)b];
    double straddle = 0.0;
    for (int64_t g = 0; g <= S; g++) {
        if (g > 0) straddle += host[(size_t)(NB + g - 1)];
        for (int r = 0; r < 2; r++)
            scores_out[2 * g + r] = (base - straddle + host[(size_t)(NB + S + 2 * g + r)]) / total;
    }
    return HICMI_OK;
}

int hicmi_p2_window_tables(hicmi_ctx* c, int64_t k, const int8_t* orders, int64_t n_orders, const uint8_t* orients,
                           int64_t n_orients)
{
    if (!c || !orders || !orients || k < 1 || k > 8 || n_orders < 1 || n_orients < 1) return fail(HICMI_EINVAL, "bad arguments");
    for (int64_t i = 0; i < n_orders * k; i++) if (orders[i] < 0 || orders[i] >= k) return fail(HICMI_EINVAL, "order table entry out of range");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure(c->d_orders, n_orders * k);
    if (!rc) rc = ensure(c->d_orients, n_orients * k);
    if (rc) return rc;
    rc = upload(c, c->d_orders, orders, (size_t)(n_orders * k));
    if (rc) return rc;
    rc = upload(c, c->d_orients, orients, (size_t)(n_orients * k));
    if (rc) return rc;
    c->tab_k = (int)k; c->n_orders = n_orders; c->n_orients = n_orients;
    c->h_orders.assign(orders, orders + n_orders * k);
    c->h_orients.assign(orients, orients + n_orients * k);
    return HICMI_OK;
}

namespace {
// candidate index of window `first`'s current configuration: identity order + the window's current signs (-1: its signs
// are not in the orientation table)
int64_t window_c0(const hicmi_ctx* c, int64_t first, int64_t k)
{
    for (int64_t r = 0; r < c->n_orients; r++) {
        bool same = true;
        for (int64_t j = 0; j < k; j++) same = same && ((c->h_orients[(size_t)(r * k + j)] != 0) == (c->h_arr_rev[(size_t)(first + j)] != 0));
        if (same) return r;
    }
    return -1;
}

struct BatchCost { int64_t g_total = 0; int max_m = 0; double g_bytes = 0.0, d_bytes = 0.0, g_flops = 0.0; };

// the batch records of `count` consecutive windows (first0, first0+1, ...) of k scaffolds against the CURRENT arrangement
int fill_batch(hicmi_ctx* c, int64_t first0, int64_t count, int64_t k, std::vector<WindowBatchEntry>& wb, BatchCost& bc)
{
    const int64_t S = (int64_t)c->h_arr_id.size();
    if (c->n_arr < 1 || S < 1) return fail(HICMI_EINVAL, "hicmi_p2_set_arrangement has not run");
    if (k != c->tab_k) return fail(HICMI_EINVAL, "hicmi_p2_window_tables has not been called for k = %lld", (long long)k);
    if (first0 < 0 || count < 1 || first0 + count - 1 + k > S) return fail(HICMI_EINVAL, "window out of range");
    const int64_t n_cand = c->n_orders * c->n_orients;
    wb.assign((size_t)count, WindowBatchEntry{});
    int64_t g_total = 0; int max_m = 0; double g_bytes = 0.0, d_bytes = 0.0, g_flops = 0.0;
    for (int64_t wdx = 0; wdx < count; wdx++) {
        const int64_t first = first0 + wdx;
        WindowBatchEntry& e = wb[(size_t)wdx];
        memset(&e, 0, sizeof(e));
        const int p0 = c->h_arr_pos[(size_t)first], p1 = c->h_arr_pos[(size_t)(first + k)];
        e.p0 = p0; e.m = p1 - p0; e.g_off = g_total;
        for (int64_t j = 0; j < k; j++) {
            const int32_t sc = c->h_arr_id[(size_t)(first + j)];
            e.w.start[j] = c->h_scaf_start[(size_t)sc];
            e.w.len[j] = c->h_scaf_len[(size_t)sc];
            e.w.off[j] = c->h_arr_pos[(size_t)(first + j)] - p0;
            e.w.rev[j] = c->h_arr_rev[(size_t)(first + j)];
        }
        g_total += (int64_t)e.m * e.m;
        max_m = std::max(max_m, e.m);
        g_bytes += 8.0 * (double)e.m * (double)(c->n_arr - e.m);
        g_flops += 2.0 * (double)e.m * (double)e.m * (double)(c->n_arr - e.m);       // A (m x (n - m)) . Toeplitz ((n - m) x m), all scaffolds of the window
        d_bytes += 8.0 * (double)n_cand * (0.5 * (double)e.m * (double)(e.m - 1) + (double)e.m);
    }
    bc.g_total = g_total; bc.max_m = max_m; bc.g_bytes = g_bytes; bc.d_bytes = d_bytes; bc.g_flops = g_flops;
    return HICMI_OK;
}

// deltas of `count` consecutive windows (first0, first0+1, ...) of k scaffolds against the CURRENT
// arrangement, one launch pair, and their copy to the pinned download buffer (count x n_cand doubles), all queued
int window_batch_enqueue(hicmi_ctx* c, int64_t first0, int64_t count, int64_t k)
{
    std::vector<WindowBatchEntry> wb;
    BatchCost bc;
    int rc = fill_batch(c, first0, count, k, wb, bc);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    const int64_t n_cand = c->n_orders * c->n_orients;
    int64_t g_total = bc.g_total; const int max_m = bc.max_m;
    const double g_bytes = bc.g_bytes, d_bytes = bc.d_bytes, g_flops = bc.g_flops;
    // placement tables (k_part2_window.hip) unless the direct per-candidate kernels are asked for (A/B switch)
    static const bool direct = getenv("HICMI_P2_WINDOW_DIRECT") != nullptr;
    if (!direct) g_total = count * window_table_doubles((int)k);
    rc = ensure(c->d_G, g_total);
    if (!rc) rc = ensure(c->d_delta, n_cand * count);
    if (!rc) rc = ensure(c->d_wb, count);
    if (rc) return rc;
    rc = upload(c, c->d_wb, wb.data(), sizeof(WindowBatchEntry) * (size_t)count);
    if (rc) return rc;
    {
        // the G and delta kernels are launched as a pair; each family is a timed region of its own
        if (!direct) { c->launches[F_P2_WINDOW_FLOPS]++; c->bytes[F_P2_WINDOW_FLOPS] += g_flops; }   // (flops of the GEMM form: bench.py's `mfma`)
        Timed t(c, F_P2_WINDOW_G, g_bytes);
        if (direct)
            launch_p2_window_batch_G(c->dM2, c->ld2, c->d_pos2sel, (int)c->n_arr, c->d_wb, (int)count, max_m, c->d_H, c->d_G, c->stream);
        else
            launch_p2_window_tables(c->dM2, c->ld2, c->d_pos2sel, (int)c->n_arr, (int)k, c->d_wb, wb.data(), (int)count, max_m,
                                    c->d_H, c->d_G, c->stream);
    }
    {
        Timed t(c, F_P2_WINDOW_DELTA, d_bytes);
        if (direct)
            launch_p2_window_batch_delta(c->dM2, c->ld2, c->d_pos2sel, (int)c->n_arr, (int)k, c->d_wb, (int)count, max_m, c->d_orders,
                                         c->d_orients, (int)c->n_orders, (int)c->n_orients, c->d_H, c->d_G, c->d_delta, c->stream);
        else
            launch_p2_window_candidates((int)k, (int)count, c->d_orders, c->d_orients, (int)c->n_orders, (int)c->n_orients, c->d_G,
                                        c->d_delta, c->stream);
    }
    HIPCHK(hipGetLastError());
    rc = ensure_pin_down(c, sizeof(double) * (size_t)(n_cand * count));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->pin_down, c->d_delta, sizeof(double) * (size_t)(n_cand * count), hipMemcpyDeviceToHost, c->stream));
    return HICMI_OK;
}

// ... and waited for; delta_out: count x n_cand
int window_batch(hicmi_ctx* c, int64_t first0, int64_t count, int64_t k, double* delta_out)
{
    int rc = window_batch_enqueue(c, first0, count, k);
    if (rc) return rc;
    HIPCHK(sync_stream(c));
    memcpy(delta_out, c->pin_down, sizeof(double) * (size_t)(c->n_orders * c->n_orients * count));
    return HICMI_OK;
}
}  // namespace

int hicmi_p2_score_window(hicmi_ctx* c, int64_t first, int64_t k, double* delta_out)
{
    if (!c || !delta_out) return fail(HICMI_EINVAL, "bad arguments");
    return window_batch(c, first, 1, k, delta_out);
}

// ---------------------------------------------------------------------------------------------------
// Whole decision steps in one call: fast scores of every candidate (device enumeration), short list
// of the candidates within 1e-9 of the step's best, literal re-scoring of the short list (cached by
// bin order under the current total), then the reference's first-strict-maximum scan (OG:349,359,
// 464,535).  The same logic as SubMatrix.first_strict_max in orderGenome.py, minus ~10 host round trips.
namespace {
const double kNearTop = 1e-9;

void use_total(hicmi_ctx* c, double total)
{
    if (!c->cache_valid || c->cache_total != total) { c->exact_cache.clear(); c->cache_total = total; c->cache_valid = true; }
}

// literal scores of rows (each n_used selection indices) under `total`, through the cache: literal_enqueue queues the
// kernel for the rows the cache does not hold and the copy of their scores to the pinned download buffer, literal_collect
// waits for them, fills the cache and reads every row's score from it
struct LiteralPending { std::vector<std::string> keys; std::vector<size_t> todo; bool queued = false; };

int literal_enqueue(hicmi_ctx* c, const std::vector<std::vector<int32_t>>& rows, double total, LiteralPending& p)
{
    p.keys.assign(rows.size(), std::string()); p.todo.clear(); p.queued = false;
    if (rows.empty()) return HICMI_OK;
    const int64_t n_used = (int64_t)rows[0].size();
    std::unordered_map<std::string, size_t> pending;
    for (size_t i = 0; i < rows.size(); i++) {
        p.keys[i].assign(reinterpret_cast<const char*>(rows[i].data()), rows[i].size() * sizeof(int32_t));
        if (c->exact_cache.count(p.keys[i]) || pending.count(p.keys[i])) continue;
        pending[p.keys[i]] = p.todo.size();
        p.todo.push_back(i);
    }
    if (p.todo.empty() || n_used < 2) return HICMI_OK;
    std::vector<int32_t> flat((size_t)n_used * p.todo.size());
    for (size_t t = 0; t < p.todo.size(); t++) memcpy(flat.data() + t * n_used, rows[p.todo[t]].data(), sizeof(int32_t) * (size_t)n_used);
    const int64_t n_cand = (int64_t)p.todo.size();
    int rc = ensure(c->d_perms, n_cand * n_used);
    if (!rc) rc = ensure(c->d_scores, n_cand);
    if (!rc) rc = ensure(c->d_T, 2 * n_cand * n_used);
    if (rc) return rc;
    rc = ensure_pin_down(c, sizeof(double) * (size_t)n_cand);
    if (rc) return rc;
    rc = upload(c, c->d_perms, flat.data(), sizeof(int32_t) * flat.size());
    if (rc) return rc;
    {
        Timed t(c, F_P2_EXACT, 8.0 * (double)n_cand * 0.5 * (double)n_used * (double)(n_used - 1));
        launch_p2_score_exact(c->dM2, c->ld2, c->d_perms, (int)n_cand, (int)n_used, total, c->d_T,
                              c->d_T + n_cand * n_used, c->d_scores, c->stream);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->pin_down, c->d_scores, sizeof(double) * (size_t)n_cand, hipMemcpyDeviceToHost, c->stream));
    p.queued = true;
    return HICMI_OK;
}

int literal_collect(hicmi_ctx* c, const LiteralPending& p, std::vector<double>& out)
{
    out.assign(p.keys.size(), 0.0);
    if (p.keys.empty()) return HICMI_OK;
    if (p.queued) HIPCHK(sync_stream(c));
    const double* vals = reinterpret_cast<const double*>(c->pin_down.get());
    for (size_t t = 0; t < p.todo.size(); t++) c->exact_cache[p.keys[p.todo[t]]] = p.queued ? vals[t] : 0.0;   // fewer than 2 bins: cost 0.0
    for (size_t i = 0; i < p.keys.size(); i++) out[i] = c->exact_cache[p.keys[i]];
    return HICMI_OK;
}

int literal_scores(hicmi_ctx* c, const std::vector<std::vector<int32_t>>& rows, double total, std::vector<double>& out)
{
    LiteralPending p;
    int rc = literal_enqueue(c, rows, total, p);
    if (rc) return rc;
    return literal_collect(c, p, out);
}

// indices of the candidates whose fast score is within kNearTop of max(best fast, floor)
void short_list(const std::vector<double>& fast, double floor, std::vector<int64_t>& near)
{
    near.clear();
    bool any = false; double top = floor;
    for (double v : fast) if (std::isfinite(v)) { any = true; if (v > top) top = v; }
    if (!any) return;
    const double thr = top - std::fabs(top) * kNearTop;
    for (size_t i = 0; i < fast.size(); i++) if (std::isfinite(fast[i]) && fast[i] >= thr) near.push_back((int64_t)i);
}
}  // namespace

namespace {
// bin orders (selection indices) of the candidates `near` of the window first .. first + k - 1 of the CURRENT arrangement
void near_rows(const hicmi_ctx* c, int64_t first, int64_t k, const std::vector<int64_t>& near, std::vector<std::vector<int32_t>>& rows)
{
    const int64_t n_ori = c->n_orients;
    const int p0 = c->h_arr_pos[(size_t)first], p1 = c->h_arr_pos[(size_t)(first + k)];
    rows.assign(near.size(), {});
    for (size_t q = 0; q < near.size(); q++) {
        const int64_t cand = near[q];
        const int8_t* ord = c->h_orders.data() + (cand / n_ori) * k;
        const uint8_t* ori = c->h_orients.data() + (cand % n_ori) * k;
        std::vector<int32_t>& row = rows[q];
        row.reserve((size_t)c->n_arr);
        row.insert(row.end(), c->h_pos2sel.begin(), c->h_pos2sel.begin() + p0);
        for (int64_t j = 0; j < k; j++) {
            const int32_t sc = c->h_arr_id[(size_t)(first + ord[j])];
            const int32_t st = c->h_scaf_start[(size_t)sc], ln = c->h_scaf_len[(size_t)sc];
            if (ori[j]) for (int32_t e = 0; e < ln; e++) row.push_back(st + ln - 1 - e);
            else        for (int32_t e = 0; e < ln; e++) row.push_back(st + e);
        }
        row.insert(row.end(), c->h_pos2sel.begin() + p1, c->h_pos2sel.end());
    }
}

// the reference's `if cost > bestCost` over a short list in enumeration order, on the literal scores `lit`
void pick_first_strict_max(const std::vector<int64_t>& near, const std::vector<double>& near_fast, const std::vector<double>& lit,
                           double floor, int64_t* pick_out, double* best_out, double* pick_fast_out)
{
    double best = floor; int64_t pick = -1; size_t pick_q = 0;
    for (size_t q = 0; q < near.size(); q++) if (lit[q] > best) { best = lit[q]; pick = near[q]; pick_q = q; }
    *pick_out = pick; *best_out = best;
    if (pick >= 0) *pick_fast_out = near_fast[pick_q];
}

// The decision of one window from its short list: `near` = the candidates within kNearTop of max(best fast, floor) in
// enumeration order, `near_fast` their fast scores, c0 the current configuration's candidate.  Shared by the host list
// (decide_from_delta) and the device list (window_near_batch).
int decide_from_near(hicmi_ctx* c, int64_t first, int64_t k, double total, double floor, double cur_fast, int64_t c0,
                     const std::vector<int64_t>& near, const std::vector<double>& near_fast, int64_t* pick_out,
                     double* best_out, double* pick_fast_out)
{
    const int64_t S = (int64_t)c->h_arr_id.size();
    *pick_out = -1; *best_out = floor; *pick_fast_out = cur_fast;
    if (near.empty()) return HICMI_OK;
    int rc;
    // The candidate that IS the current arrangement is near the top in every window (its fast score is the floor's twin)
    // and its bin order is the same in all of them: its literal score is worked out once per arrangement and total, not
    // through a 7 KB row and cache key per window (138 windows x 1-2 rounds per chromosome at 16k: ~3 ms of a 4.5 ms scan).
    double lit_c0 = 0.0; bool have_c0 = false;
    if (k != S) {
        for (int64_t cand : near) if (cand == c0) have_c0 = true;
        if (have_c0) {
            if (c->cur_lit_version != c->arr_version || c->cur_lit_total != total) {
                std::vector<std::vector<int32_t>> one(1, c->h_pos2sel);
                std::vector<double> v;
                rc = literal_scores(c, one, total, v);
                if (rc) return rc;
                c->cur_lit_version = c->arr_version; c->cur_lit_total = total; c->cur_lit_value = v[0];
            }
            lit_c0 = c->cur_lit_value;
            if (near.size() == 1) {                          // nothing but the arrangement itself: decided
                if (lit_c0 > floor) { *pick_out = c0; *best_out = lit_c0; *pick_fast_out = near_fast[0]; }
                return HICMI_OK;
            }
        }
    }
    // (the arrangement's own row is not built and keyed again: it has the same bin order, hence the same cache key and value)
    std::vector<int64_t> others;
    for (int64_t cand : near) if (!(have_c0 && cand == c0)) others.push_back(cand);
    std::vector<std::vector<int32_t>> rows;
    near_rows(c, first, k, others, rows);
    std::vector<double> lit_others;
    rc = literal_scores(c, rows, total, lit_others);
    if (rc) return rc;
    std::vector<double> lit(near.size());
    for (size_t q = 0, o = 0; q < near.size(); q++) lit[q] = (have_c0 && near[q] == c0) ? lit_c0 : lit_others[o++];
    pick_first_strict_max(near, near_fast, lit, floor, pick_out, best_out, pick_fast_out);
    return HICMI_OK;
}

// the decision of one window from its deltas; cur_fast (fast score of the current arrangement) is
// computed on first use when NaN
int decide_from_delta(hicmi_ctx* c, int64_t first, int64_t k, double total, double floor, double& cur_fast,
                      const double* delta, int64_t* pick_out, double* best_out, double* pick_fast_out)
{
    const int64_t S = (int64_t)c->h_arr_id.size();
    const int64_t n_ord = c->n_orders, n_ori = c->n_orients, n_cand = n_ord * n_ori;
    *pick_out = -1; *best_out = floor; *pick_fast_out = cur_fast;
    const int64_t c0 = window_c0(c, first, k);
    if (c0 < 0) return fail(HICMI_EINVAL, "current orientation not in the orientation table");
    std::vector<double> fast((size_t)n_cand);
    int rc;
    if (k == S) for (int64_t i = 0; i < n_cand; i++) fast[(size_t)i] = delta[(size_t)i] / total;
    else {
        if (std::isnan(cur_fast)) { rc = hicmi_p2_arrangement_score(c, total, &cur_fast); if (rc) return rc; }
        for (int64_t i = 0; i < n_cand; i++) fast[(size_t)i] = cur_fast + (delta[(size_t)i] - delta[(size_t)c0]) / total;
    }
    std::vector<int64_t> near;
    short_list(fast, floor, near);
    std::vector<double> near_fast(near.size());
    for (size_t q = 0; q < near.size(); q++) near_fast[q] = fast[(size_t)near[q]];
    return decide_from_near(c, first, k, total, floor, cur_fast, c0, near, near_fast, pick_out, best_out, pick_fast_out);
}

// Short lists of `count` consecutive windows of k scaffolds against the CURRENT arrangement, from the device
// (k_win_near): per window its near-top candidates in enumeration order and their fast scores, equal to short_list over
// the downloaded deltas.  All windows share floor and cur_fast (NaN: computed here when k < S).  n_near[w] > cap: the
// window's list overflowed, near[w] / near_fast[w] are left empty.
// window_near_enqueue queues the kernels and the copy of every window's count and of the first kNearHead entries of its
// list to the pinned download buffer; window_near_collect waits for them ONCE and goes back to the device only for a
// list that is longer.  Device work area: [pass-1 partials][per-window counters][NearEntry lists] - the counters lie
// directly in front of the lists, so that a single window's count and list head come down in one copy.
const int64_t kNearHead = 16;

struct NearPending { int64_t count = 0, cap = 0, head = 0; size_t off_cnt = 0, off_list = 0, host_list = 0; };

int window_near_enqueue(hicmi_ctx* c, int64_t first0, int64_t count, int64_t k, double total, double floor, double& cur_fast,
                        int64_t cap, NearPending& p)
{
    std::vector<WindowBatchEntry> wb;
    BatchCost bc;
    int rc = fill_batch(c, first0, count, k, wb, bc);
    if (rc) return rc;
    if (k > 8 || cap < 1 || cap > (1 << 24)) return fail(HICMI_EINVAL, "short lists take k <= 8 and 1 <= cap <= 2^24");
    const int64_t S = (int64_t)c->h_arr_id.size();
    for (int64_t wdx = 0; wdx < count; wdx++) {
        const int64_t c0 = window_c0(c, first0 + wdx, k);
        if (c0 < 0) return fail(HICMI_EINVAL, "current orientation not in the orientation table");
        wb[(size_t)wdx].c0 = (int32_t)c0;
    }
    if (k != S && std::isnan(cur_fast)) { rc = hicmi_p2_arrangement_score(c, total, &cur_fast); if (rc) return rc; }
    HIPCHK(hipSetDevice(c->device));
    const int n_blocks = window_near_blocks((int)c->n_orders);
    const size_t off_cnt = (size_t)count * (size_t)n_blocks * sizeof(double);
    const size_t off_list = off_cnt + (((size_t)count * sizeof(int32_t) + 15) & ~(size_t)15);
    const size_t bytes = off_list + (size_t)count * (size_t)cap * sizeof(NearEntry);
    rc = ensure(c->d_G, count * window_table_doubles((int)k));
    if (!rc) rc = ensure(c->d_wnear, (int64_t)bytes);
    if (!rc) rc = ensure(c->d_wb, count);
    if (rc) return rc;
    rc = upload(c, c->d_wb, wb.data(), sizeof(WindowBatchEntry) * (size_t)count);
    if (rc) return rc;
    int32_t* d_count = reinterpret_cast<int32_t*>(c->d_wnear + off_cnt);
    NearEntry* d_list = reinterpret_cast<NearEntry*>(c->d_wnear + off_list);
    {
        c->launches[F_P2_WINDOW_FLOPS]++; c->bytes[F_P2_WINDOW_FLOPS] += bc.g_flops;
        Timed t(c, F_P2_WINDOW_G, bc.g_bytes);
        launch_p2_window_near(c->dM2, c->ld2, c->d_pos2sel, (int)c->n_arr, (int)k, c->d_wb, wb.data(), (int)count, bc.max_m,
                              c->d_orders, c->d_orients, (int)c->n_orders, (int)c->n_orients, c->d_H, c->d_G, k == S ? 1 : 0,
                              total, cur_fast, floor, kNearTop, reinterpret_cast<double*>(c->d_wnear.get()), d_count,
                              d_list, (int)cap, c->stream);
    }
    HIPCHK(hipGetLastError());
    p.count = count; p.cap = cap; p.head = std::min<int64_t>(kNearHead, cap); p.off_cnt = off_cnt; p.off_list = off_list;
    p.host_list = off_list - off_cnt;                       // pinned buffer: [counters, padded][count x head entries]
    const size_t row = (size_t)p.head * sizeof(NearEntry);
    rc = ensure_pin_down(c, p.host_list + row * (size_t)count);
    if (rc) return rc;
    if (count == 1)
        HIPCHK(hipMemcpyAsync(c->pin_down, d_count, p.host_list + row, hipMemcpyDeviceToHost, c->stream));
    else {
        HIPCHK(hipMemcpyAsync(c->pin_down, d_count, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpy2DAsync(c->pin_down + p.host_list, row, d_list, (size_t)cap * sizeof(NearEntry), row, (size_t)count,
                                hipMemcpyDeviceToHost, c->stream));
    }
    return HICMI_OK;
}

int window_near_collect(hicmi_ctx* c, const NearPending& p, std::vector<int64_t>& n_near,
                        std::vector<std::vector<int64_t>>& near, std::vector<std::vector<double>>& near_fast)
{
    const int64_t count = p.count, cap = p.cap;
    HIPCHK(sync_stream(c));
    std::vector<int32_t> cnt((size_t)count);
    memcpy(cnt.data(), c->pin_down, sizeof(int32_t) * (size_t)count);
    n_near.assign((size_t)count, 0); near.assign((size_t)count, {}); near_fast.assign((size_t)count, {});
    int64_t widest = 0;
    for (int64_t w = 0; w < count; w++) {
        n_near[(size_t)w] = cnt[(size_t)w];
        if (cnt[(size_t)w] <= cap) widest = std::max<int64_t>(widest, cnt[(size_t)w]);
    }
    if (widest == 0) return HICMI_OK;
    size_t row = (size_t)p.head * sizeof(NearEntry);
    const char* lists = c->pin_down + p.host_list;
    if (widest > p.head) {
        // a list beyond the head: the first `widest` entries of every window in one strided copy
        row = (size_t)widest * sizeof(NearEntry);
        int rc = ensure_pin_down(c, row * (size_t)count);
        if (rc) return rc;
        HIPCHK(hipMemcpy2DAsync(c->pin_down, row, c->d_wnear + p.off_list, (size_t)cap * sizeof(NearEntry), row, (size_t)count,
                                hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_stream(c));
        lists = c->pin_down;
    }
    std::vector<NearEntry> ent;
    for (int64_t w = 0; w < count; w++) {
        const int64_t m = cnt[(size_t)w];
        if (m < 1 || m > cap) continue;
        const NearEntry* src = reinterpret_cast<const NearEntry*>(lists + row * (size_t)w);
        ent.assign(src, src + m);
        std::sort(ent.begin(), ent.end(), [](const NearEntry& a, const NearEntry& b) { return a.cand < b.cand; });
        near[(size_t)w].resize((size_t)m); near_fast[(size_t)w].resize((size_t)m);
        for (int64_t q = 0; q < m; q++) { near[(size_t)w][(size_t)q] = ent[(size_t)q].cand; near_fast[(size_t)w][(size_t)q] = ent[(size_t)q].fast; }
    }
    return HICMI_OK;
}

int window_near_batch(hicmi_ctx* c, int64_t first0, int64_t count, int64_t k, double total, double floor, double& cur_fast,
                      int64_t cap, std::vector<int64_t>& n_near, std::vector<std::vector<int64_t>>& near,
                      std::vector<std::vector<double>>& near_fast)
{
    NearPending p;
    int rc = window_near_enqueue(c, first0, count, k, total, floor, cur_fast, cap, p);
    if (rc) return rc;
    return window_near_collect(c, p, n_near, near, near_fast);
}

const int64_t kNearCap = 4096;     // candidates per window list; a window beyond it sends its batch down the delta path

int check_window_call(hicmi_ctx* c, int64_t first, int64_t k)
{
    const int64_t S = (int64_t)c->h_arr_id.size();
    if (c->n_arr < 1 || S < 1) return fail(HICMI_EINVAL, "hicmi_p2_set_arrangement has not run");
    if (k != c->tab_k || c->h_orders.empty()) return fail(HICMI_EINVAL, "hicmi_p2_window_tables has not been called for k = %lld", (long long)k);
    if (first < 0 || first + k > S) return fail(HICMI_EINVAL, "window out of range");
    for (int64_t j = 0; j < k; j++) if (c->h_orders[(size_t)j] != j) return fail(HICMI_EINVAL, "orders[0] must be the identity");
    return HICMI_OK;
}
}  // namespace

int hicmi_p2_decide_window(hicmi_ctx* c, int64_t first, int64_t k, double total, double floor, double cur_fast,
                           int64_t* pick_out, double* best_out, double* pick_fast_out)
{
    if (!c || !pick_out || !best_out || !pick_fast_out) return fail(HICMI_EINVAL, "NULL argument");
    int rc = check_window_call(c, first, k);
    if (rc) return rc;
    use_total(c, total);
    if (k >= c->near_min_k) {
        std::vector<int64_t> n_near; std::vector<std::vector<int64_t>> near; std::vector<std::vector<double>> near_fast;
        rc = window_near_batch(c, first, 1, k, total, floor, cur_fast, kNearCap, n_near, near, near_fast);
        if (rc) return rc;
        if (n_near[0] <= kNearCap)
            return decide_from_near(c, first, k, total, floor, cur_fast, window_c0(c, first, k), near[0], near_fast[0],
                                    pick_out, best_out, pick_fast_out);
    }
    std::vector<double> delta((size_t)(c->n_orders * c->n_orients));
    rc = window_batch(c, first, 1, k, delta.data());
    if (rc) return rc;
    return decide_from_delta(c, first, k, total, floor, cur_fast, delta.data(), pick_out, best_out, pick_fast_out);
}

int hicmi_p2_window_shortlist(hicmi_ctx* c, int64_t first, int64_t count, int64_t k, double total, double floor,
                              double cur_fast, int64_t cap, int64_t* n_near_out, int64_t* idx_out, double* fast_out)
{
    if (!c || !n_near_out || !idx_out || !fast_out || count < 1) return fail(HICMI_EINVAL, "bad arguments");
    int rc = check_window_call(c, first, k);
    if (rc) return rc;
    std::vector<int64_t> n_near; std::vector<std::vector<int64_t>> near; std::vector<std::vector<double>> near_fast;
    rc = window_near_batch(c, first, count, k, total, floor, cur_fast, cap, n_near, near, near_fast);
    if (rc) return rc;
    for (int64_t w = 0; w < count; w++) {
        n_near_out[w] = n_near[(size_t)w];
        for (size_t q = 0; q < near[(size_t)w].size(); q++) {
            idx_out[w * cap + (int64_t)q] = near[(size_t)w][q];
            fast_out[w * cap + (int64_t)q] = near_fast[(size_t)w][q];
        }
    }
    return HICMI_OK;
}

int hicmi_p2_decide_insertion(hicmi_ctx* c, const int32_t* ids, const uint8_t* rev, int64_t S, int32_t new_id,
                              int32_t new_rev_now, int64_t* gap_out, int32_t* rev_out, double* best_out)
{
    if (!c || !ids || !rev || !gap_out || !rev_out || !best_out || S < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n_scaf < 1) return fail(HICMI_EINVAL, "hicmi_p2_layout has not run");
    if (new_id < 0 || new_id >= c->n_scaf) return fail(HICMI_EINVAL, "new scaffold out of range");
    *gap_out = -1; *rev_out = 0; *best_out = 0.0;
    // total of the sub-matrix in the order "ordered scaffolds, then the new one" (OG:484-487 -> OG:343)
    std::vector<int32_t> ids2(ids, ids + S); ids2.push_back(new_id);
    std::vector<uint8_t> rev2(rev, rev + S); rev2.push_back(new_rev_now ? 1 : 0);
    int rc = hicmi_p2_set_arrangement(c, ids2.data(), rev2.data(), S + 1);
    if (rc) return rc;
    double total = 0.0;
    rc = hicmi_p2_arrangement_total(c, &total);
    if (rc) return rc;
    use_total(c, total);
    rc = hicmi_p2_set_arrangement(c, ids, rev, S);
    if (rc) return rc;
    const int64_t gaps = S + 1;
    std::vector<double> by_gap_rev((size_t)(2 * gaps));
    rc = hicmi_p2_score_insertions(c, new_id, total, by_gap_rev.data());
    if (rc) return rc;
    // enumeration order of OG:344-365: gap i tests the current orientation, then the flipped one, and the
    // scaffold stays flipped for the next gap
    std::vector<double> fast((size_t)(2 * gaps));
    std::vector<int32_t> tag_rev((size_t)(2 * gaps));
    int32_t o = new_rev_now ? 1 : 0;
    for (int64_t i = 0; i < gaps; i++) {
        tag_rev[(size_t)(2 * i)] = o; tag_rev[(size_t)(2 * i + 1)] = o ^ 1;
        fast[(size_t)(2 * i)] = by_gap_rev[(size_t)(2 * i + o)];
        fast[(size_t)(2 * i + 1)] = by_gap_rev[(size_t)(2 * i + (o ^ 1))];
        o ^= 1;
    }
    std::vector<int64_t> near;
    short_list(fast, 0.0, near);
    if (near.empty()) return HICMI_OK;
    const int32_t st = c->h_scaf_start[(size_t)new_id], ln = c->h_scaf_len[(size_t)new_id];
    std::vector<std::vector<int32_t>> rows(near.size());
    for (size_t q = 0; q < near.size(); q++) {
        const int64_t g = near[q] / 2;
        const int32_t r = tag_rev[(size_t)near[q]];
        const int P = c->h_arr_pos[(size_t)g];
        std::vector<int32_t>& row = rows[q];
        row.reserve((size_t)(c->n_arr + ln));
        row.insert(row.end(), c->h_pos2sel.begin(), c->h_pos2sel.begin() + P);
        if (r) for (int32_t e = 0; e < ln; e++) row.push_back(st + ln - 1 - e);
        else   for (int32_t e = 0; e < ln; e++) row.push_back(st + e);
        row.insert(row.end(), c->h_pos2sel.begin() + P, c->h_pos2sel.end());
    }
    std::vector<double> lit;
    rc = literal_scores(c, rows, total, lit);
    if (rc) return rc;
    double best = 0.0; int64_t pick = -1;
    for (size_t q = 0; q < near.size(); q++) if (lit[q] > best) { best = lit[q]; pick = near[q]; }
    if (pick >= 0) { *gap_out = pick / 2; *rev_out = tag_rev[(size_t)pick]; *best_out = best; }
    return HICMI_OK;
}


// Whole loops of the search, so that a chromosome costs a handful of host calls (several chromosomes
// run concurrently from host threads, each on its own context).
namespace {
void apply_insertion(int32_t* ids, uint8_t* rev, int64_t& S, int64_t gap, int32_t new_id, int32_t r)
{
    for (int64_t j = S; j > gap; j--) { ids[j] = ids[j - 1]; rev[j] = rev[j - 1]; }
    ids[gap] = new_id; rev[gap] = (uint8_t)(r ? 1 : 0);
    S++;
}

struct InsJob {
    hicmi_ctx* c; int32_t* ids; uint8_t* rev; int64_t S; const int32_t* new_ids; int64_t n_new;
    int64_t t = 0; double best = 0.0; bool device_ok = true;
};

// Queue the remaining insertions of every job in lock step on `lead`'s stream, with the decisions taken on
// the device (k_part2_insert.hip), and synchronise once.  Decided steps are applied to ids/rev/S/t of each
// job; a job stops early at a step the device declined (short list longer than the cap), which the host
// has to decide.
int queue_insertions(hicmi_ctx* lead, const std::vector<InsJob*>& jobs)
{
    const int nj = (int)jobs.size();
    if (nj == 0) return HICMI_OK;
    const int NB = kBaseSlabs;
    static const int max_c = getenv("HICMI_P2_INS_MAXC") ? atoi(getenv("HICMI_P2_INS_MAXC")) : INS_MAXC;   // tests: force host steps
    int64_t steps_max = 0;
    std::vector<size_t> blob_off((size_t)nj);
    size_t blob_bytes = 0;
    for (int j = 0; j < nj; j++) {
        InsJob& job = *jobs[(size_t)j];
        hicmi_ctx* c = job.c;
        int rc = hicmi_p2_set_arrangement(c, job.ids, job.rev, job.S);
        if (rc) return rc;
        if (c != lead) HIPCHK(sync_stream(c));             // the queue runs on lead's stream
        const int64_t n_steps = job.n_new - job.t;
        int64_t n_max = c->n_arr;
        for (int64_t t = 0; t < n_steps; t++) n_max += c->h_scaf_len[(size_t)job.new_ids[job.t + t]];
        rc = check_candidate_bins(n_max);
        if (rc) return rc;
        const int64_t S_max = job.S + n_steps;
        rc = ensure(c->d_arr_packed2, 3 * std::max<int64_t>(S_max, c->n_scaf) + 2);
        if (!rc) rc = ensure(c->d_pos2sel2, c->n2);
        if (!rc) rc = ensure(c->d_ins_T, (1 + 2 * (int64_t)INS_MAXC) * n_max);
        if (!rc) rc = ensure(c->d_ins_partial, NB + n_max + 2 * (S_max + 1));
        if (rc) return rc;
        steps_max = std::max(steps_max, n_steps);
        blob_off[(size_t)j] = blob_bytes;
        blob_bytes += (sizeof(InsState) + sizeof(InsLog) * (size_t)n_steps + 15) & ~(size_t)15;
    }
    HIPCHK(hipSetDevice(lead->device));
    int rc = ensure(lead->d_ins_blob, (int64_t)blob_bytes);
    if (!rc) rc = ensure(lead->d_ins_steps, steps_max * nj);
    if (rc) return rc;
    // one record per (step, job); sizes per step for the launch grids
    std::vector<InsStep> table((size_t)(steps_max * nj));
    std::vector<int> max_n_used((size_t)steps_max, 0), max_S((size_t)steps_max, 0), max_n_arr((size_t)steps_max, 0);
    double algo = 0.0;
    for (int j = 0; j < nj; j++) {
        InsJob& job = *jobs[(size_t)j];
        hicmi_ctx* c = job.c;
        const int64_t n_steps = job.n_new - job.t;
        int64_t n_max = c->n_arr;
        for (int64_t t = 0; t < n_steps; t++) n_max += c->h_scaf_len[(size_t)job.new_ids[job.t + t]];
        InsState* st = reinterpret_cast<InsState*>(lead->d_ins_blob + blob_off[(size_t)j]);
        InsLog* log = reinterpret_cast<InsLog*>(lead->d_ins_blob + blob_off[(size_t)j] + sizeof(InsState));
        int32_t* packed[2] = {c->d_arr_packed, c->d_arr_packed2};
        int32_t* pos2sel[2] = {c->d_pos2sel, c->d_pos2sel2};
        int64_t n_arr = c->n_arr;
        for (int64_t t = 0; t < steps_max; t++) {
            InsStep& d = table[(size_t)(t * nj + j)];
            memset(&d, 0, sizeof(d));
            d.st = st;
            if (t >= n_steps) continue;                       // this chromosome has finished: inactive record
            const int cur = (int)(t & 1), nxt = cur ^ 1;
            const int32_t nid = job.new_ids[job.t + t];
            const int L = c->h_scaf_len[(size_t)nid];
            d.M2 = c->dM2; d.H = c->d_H; d.ld2 = c->ld2;
            d.pos_cur = pos2sel[cur]; d.pos_nxt = pos2sel[nxt]; d.packed_cur = packed[cur]; d.packed_nxt = packed[nxt];
            d.T_total = c->d_ins_T; d.T_cand = c->d_ins_T + n_max; d.work = c->d_ins_T + (1 + (int64_t)INS_MAXC) * n_max;
            d.partial = c->d_ins_partial; d.log = log + t;
            d.n_arr = (int32_t)n_arr; d.S = (int32_t)(job.S + t); d.L = L; d.new_start = c->h_scaf_start[(size_t)nid];
            d.new_id = nid; d.active = 1; d.step = (int32_t)t; d.last = t == n_steps - 1;
            max_n_used[(size_t)t] = std::max(max_n_used[(size_t)t], (int)(n_arr + L));
            max_S[(size_t)t] = std::max(max_S[(size_t)t], d.S);
            max_n_arr[(size_t)t] = std::max(max_n_arr[(size_t)t], (int)n_arr);
            const double nn = (double)n_arr, Ld = (double)L, sd = (double)d.S;
            algo += 8.0 * (0.5 * nn * (nn - 1.0) + nn * nn + 2.0 * (sd + 1.0) * Ld * nn) + 4.0 * (nn + Ld) * (nn + Ld);
            n_arr += L;
        }
    }
    rc = upload(lead, lead->d_ins_steps, table.data(), sizeof(InsStep) * table.size());
    if (rc) return rc;
    {
        Timed timed(lead, F_P2_INSERT, algo);
        launch_insb_reset(lead->d_ins_steps, nj, lead->stream);
        for (int64_t t = 0; t < steps_max; t++) {
            const InsStep* st_t = lead->d_ins_steps + t * nj;
            const int nu = max_n_used[(size_t)t];
            launch_insb_fast(st_t, nj, max_S[(size_t)t], max_n_arr[(size_t)t], NB, lead->stream);
            launch_insb_shortlist(st_t, nj, max_S[(size_t)t], max_n_arr[(size_t)t], NB, kNearTop, max_c, lead->stream);
            launch_insb_diag_cand(st_t, nj, nu, lead->stream);
            launch_insb_cost(st_t, nj, nu, lead->stream);
            launch_insb_apply(st_t, nj, nu, lead->stream);
        }
    }
    HIPCHK(hipGetLastError());
    std::vector<unsigned char> blob(blob_bytes);
    rc = download(lead, blob.data(), lead->d_ins_blob, blob_bytes);
    if (rc) return rc;
    if (getenv("HICMI_PART2_PROFILE")) {                   // how many lock steps needed a literal tie-break at all
        int64_t hist[5] = {0, 0, 0, 0, 0}, all_direct = 0;       // [0] = taken directly (one candidate near the top)
        for (int64_t t = 0; t < steps_max; t++) {
            int mx = -1, ran = 0;
            for (int j = 0; j < nj; j++) {
                if (t >= jobs[(size_t)j]->n_new - jobs[(size_t)j]->t) continue;
                const InsState* hs = reinterpret_cast<const InsState*>(blob.data() + blob_off[(size_t)j]);
                if (hs->fail >= 0 && t >= hs->fail) continue;         // declined: this and the later logs were never written
                const InsLog* hl = reinterpret_cast<const InsLog*>(blob.data() + blob_off[(size_t)j] + sizeof(InsState));
                const int ns = hl[t].n_short;
                hist[ns < 0 ? 0 : (ns > 3 ? 4 : ns + 1)]++;
                mx = std::max(mx, ns);
                ran++;
            }
            if (ran && mx < 0) all_direct++;
        }
        fprintf(stderr, "[hicmi] insertion short lists: direct %lld, literal with 0:%lld 1:%lld 2:%lld 3+:%lld candidates; "
                        "lock steps without any literal pass: %lld of %lld\n",
                (long long)hist[0], (long long)hist[1], (long long)hist[2], (long long)hist[3], (long long)hist[4],
                (long long)all_direct, (long long)steps_max);
    }
    for (int j = 0; j < nj; j++) {
        InsJob& job = *jobs[(size_t)j];
        const int64_t n_steps = job.n_new - job.t;
        const InsState* hst = reinterpret_cast<const InsState*>(blob.data() + blob_off[(size_t)j]);
        const InsLog* hlog = reinterpret_cast<const InsLog*>(blob.data() + blob_off[(size_t)j] + sizeof(InsState));
        const int64_t done = hst->fail >= 0 ? std::min<int64_t>(hst->fail, n_steps) : n_steps;
        for (int64_t t = 0; t < done; t++) {
            if (hlog[t].gap < 0 || hlog[t].gap > job.S) return fail(HICMI_ESTATE, "insertion log out of range");
            apply_insertion(job.ids, job.rev, job.S, hlog[t].gap, job.new_ids[job.t + t], hlog[t].rev);
            job.best = hlog[t].best;
        }
        job.t += done;
        // the device buffers hold a different arrangement from the host mirrors now
        hicmi_ctx* c = job.c;
        c->n_arr = 0; c->h_arr_id.clear(); c->h_arr_rev.clear(); c->h_arr_pos.clear(); c->h_pos2sel.clear();
    }
    return HICMI_OK;
}

int check_insert_job(const InsJob& job, int64_t S0)
{
    hicmi_ctx* c = job.c;
    if (!c || !job.ids || !job.rev || !job.new_ids || S0 < 1 || job.n_new < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (c->n_scaf < 1) return fail(HICMI_EINVAL, "hicmi_p2_layout has not run");
    std::vector<uint8_t> used((size_t)c->n_scaf, 0);
    for (int64_t j = 0; j < S0 + job.n_new; j++) {
        const int32_t v = j < S0 ? job.ids[j] : job.new_ids[j - S0];
        if (v < 0 || v >= c->n_scaf || used[(size_t)v]) return fail(HICMI_EINVAL, "scaffolds must be distinct members of the layout");
        used[(size_t)v] = 1;
    }
    return HICMI_OK;
}

int host_insertion_step(InsJob& job)
{
    int64_t gap = -1; int32_t r = 0;
    int rc = hicmi_p2_decide_insertion(job.c, job.ids, job.rev, job.S, job.new_ids[job.t], 0, &gap, &r, &job.best);
    if (rc) return rc;
    if (gap < 0) { gap = 0; r = 0; job.best = 0.0; }
    apply_insertion(job.ids, job.rev, job.S, gap, job.new_ids[job.t], r);
    job.t++;
    return HICMI_OK;
}

int run_insert_jobs(std::vector<InsJob>& all)
{
    static const bool host_only = getenv("HICMI_P2_HOST_INSERT") != nullptr;     // A/B switch: every step decided by the host
    for (InsJob& job : all) {
        int rc = check_insert_job(job, job.S);
        if (rc) return rc;
        if (job.S + job.n_new + 1 > 8192) job.device_ok = false;   // prefix table of k_insb_shortlist; the host path has no such limit
    }
    while (true) {
        std::vector<InsJob*> todo;
        for (InsJob& job : all) if (job.t < job.n_new && job.device_ok && !host_only) todo.push_back(&job);
        if (!todo.empty()) {
            int rc = queue_insertions(todo[0]->c, todo);
            if (rc) return rc;
        }
        bool pending = false;
        for (InsJob& job : all) {
            if (job.t >= job.n_new) continue;
            // the device declined this step (or may not be used): the host decides it
            do {
                int rc = host_insertion_step(job);
                if (rc) return rc;
            } while (job.t < job.n_new && (host_only || !job.device_ok));
            if (job.t < job.n_new) pending = true;
        }
        if (!pending) break;
    }
    return HICMI_OK;
}
}  // namespace

int hicmi_p2_insert_all(hicmi_ctx* c, int32_t* ids, uint8_t* rev, int64_t S0, const int32_t* new_ids, int64_t n_new,
                        double* best_out)
{
    // orderRemainderScaffolds (OG:475-493) for n_new >= 1 scaffolds pulled in order: ids/rev hold S0 entries
    // on entry and S0 + n_new on return (capacity is the caller's).  Each new scaffold enters in '+'
    // orientation (it has never been flipped, OG:265) and leaves checkAllScores in the winning
    // orientation - '+' when nothing scored above 0 (OG:341, 367-368) - at the winning gap (0 by default).
    if (!c || !best_out) return fail(HICMI_EINVAL, "bad arguments");
    std::vector<InsJob> jobs(1);
    jobs[0].c = c; jobs[0].ids = ids; jobs[0].rev = rev; jobs[0].S = S0; jobs[0].new_ids = new_ids; jobs[0].n_new = n_new;
    int rc = run_insert_jobs(jobs);
    if (rc) return rc;
    *best_out = jobs[0].best;
    return HICMI_OK;
}

int hicmi_p2_insert_all_multi(int64_t n_jobs, hicmi_ctx* const* ctxs, int32_t* const* ids, uint8_t* const* rev,
                              const int64_t* S0, const int32_t* const* new_ids, const int64_t* n_new, double* best_out)
{
    // the same for several chromosomes (one context each, all on one device), advanced in lock step: one
    // launch per kernel and step serves every chromosome that still has scaffolds to place
    if (n_jobs < 1 || !ctxs || !ids || !rev || !S0 || !new_ids || !n_new || !best_out) return fail(HICMI_EINVAL, "bad arguments");
    std::vector<InsJob> jobs((size_t)n_jobs);
    for (int64_t j = 0; j < n_jobs; j++) {
        InsJob& job = jobs[(size_t)j];
        job.c = ctxs[j]; job.ids = ids[j]; job.rev = rev[j]; job.S = S0[j]; job.new_ids = new_ids[j]; job.n_new = n_new[j];
        if (int rc = check_job_context(ctxs, j)) return rc;
    }
    int rc = run_insert_jobs(jobs);
    if (rc) return rc;
    for (int64_t j = 0; j < n_jobs; j++) best_out[j] = jobs[(size_t)j].best;
    return HICMI_OK;
}

// Placement support and break support are "table jobs": per job (chromosome) a table of closed-form scores, and per
// scaffold of its arrangement the pick among the competing candidates (pick_first_max_256, hicmi_internal.h) as an int32
// pair.  run_table_jobs is the driver of both - one record upload, one launch and one download for all jobs - and a
// TableOps holds what differs between them.
extern "C++" {
namespace {
template <typename Rec>
struct TableOps {
    int64_t max_S;                                         // scaffolds per chromosome; 0: no limit
    DevBuf<Rec> hicmi_ctx::*recs;                            // the lead context's record buffer
    // job j, its arrangement set: the length of its table, the doubles it needs in d_ins_partial, its records
    std::function<void(int64_t j, int64_t& n_table, int64_t& scratch, int64_t& n_rec)> size;
    // job j's records appended and its work added to algo; d_scores, d_best: its table and its pairs on the device
    std::function<int(int64_t j, double* d_scores, int32_t* d_best, std::vector<Rec>& recs, double& algo)> append;
    std::function<void(const Rec* d_recs, int n_rec)> launch;
};

template <typename Rec>
int run_table_jobs(int64_t n_jobs, hicmi_ctx* const* ctxs, const int32_t* const* ids, const uint8_t* const* rev,
                   const int64_t* S, const double* totals, double* const* scores_out, int32_t* const* best_out,
                   const TableOps<Rec>& ops)
{
    hicmi_ctx* lead = ctxs[0];
    std::vector<size_t> out_off((size_t)n_jobs, 0);
    std::vector<int64_t> n_table((size_t)n_jobs, 0);
    std::vector<uint8_t> run((size_t)n_jobs, 0);
    size_t blob_bytes = 0;
    int64_t n_rec = 0;
    for (int64_t j = 0; j < n_jobs; j++) {
        int rc = check_job_context(ctxs, j);
        if (rc) return rc;
        hicmi_ctx* c = ctxs[j];
        if (!ids[j] || !rev[j] || !scores_out[j] || !best_out[j] || S[j] < 1) return fail(HICMI_EINVAL, "bad arguments");
        if (ops.max_S && S[j] > ops.max_S) return fail(HICMI_EUNSUPPORTED, "more than %d scaffolds in one chromosome", (int)ops.max_S);
        rc = hicmi_p2_set_arrangement(c, ids[j], rev[j], S[j]);
        if (rc) return rc;
        if (c != lead) HIPCHK(sync_stream(c));             // the launches run on lead's stream
        rc = check_candidate_bins(c->n_arr);
        if (rc) return rc;
        int64_t scratch = 0, n_rec_j = 0;
        ops.size(j, n_table[(size_t)j], scratch, n_rec_j);
        // fewer than 2 bins, no contacts or no record: every score is 0.0 and there is no candidate
        for (int64_t i = 0; i < n_table[(size_t)j]; i++) scores_out[j][i] = 0.0;
        for (int64_t i = 0; i < S[j]; i++) { best_out[j][2 * i] = -1; best_out[j][2 * i + 1] = 0; }
        if (c->n_arr < 2 || !(totals[j] > 0.0) || n_rec_j == 0) continue;
        run[(size_t)j] = 1;
        rc = ensure(c->d_ins_partial, scratch);
        if (rc) return rc;
        out_off[(size_t)j] = blob_bytes;
        blob_bytes += ((size_t)n_table[(size_t)j] * sizeof(double) + (size_t)(2 * S[j]) * sizeof(int32_t) + 15) & ~(size_t)15;
        n_rec += n_rec_j;
    }
    if (n_rec == 0) return HICMI_OK;
    HIPCHK(hipSetDevice(lead->device));
    int rc = ensure(lead->d_ins_blob, (int64_t)blob_bytes);
    if (!rc) rc = ensure(lead->*ops.recs, n_rec);
    if (rc) return rc;
    std::vector<Rec> recs;
    recs.reserve((size_t)n_rec);
    double algo = 0.0;
    for (int64_t j = 0; j < n_jobs; j++) {
        if (!run[(size_t)j]) continue;
        double* d_scores = reinterpret_cast<double*>(lead->d_ins_blob + out_off[(size_t)j]);
        rc = ops.append(j, d_scores, reinterpret_cast<int32_t*>(d_scores + n_table[(size_t)j]), recs, algo);
        if (rc) return rc;
    }
    rc = upload(lead, lead->*ops.recs, recs.data(), sizeof(Rec) * recs.size());
    if (rc) return rc;
    {
        Timed timed(lead, F_P2_INSERT, algo);
        ops.launch(lead->*ops.recs, (int)n_rec);
    }
    HIPCHK(hipGetLastError());
    std::vector<unsigned char> blob(blob_bytes);
    rc = download(lead, blob.data(), lead->d_ins_blob, blob_bytes);
    if (rc) return rc;
    for (int64_t j = 0; j < n_jobs; j++) {
        if (!run[(size_t)j]) continue;
        const size_t nd = (size_t)n_table[(size_t)j];
        memcpy(scores_out[j], blob.data() + out_off[(size_t)j], nd * sizeof(double));
        memcpy(best_out[j], blob.data() + out_off[(size_t)j] + nd * sizeof(double), (size_t)(2 * S[j]) * sizeof(int32_t));
    }
    return HICMI_OK;
}
}  // namespace
}  // extern "C++"

// Placement support (k_part2_support.hip): every scaffold of every job's arrangement taken out and scored at every gap
// in both orientations, one record per (job, scaffold).
int hicmi_p2_support_multi(int64_t n_jobs, hicmi_ctx* const* ctxs, const int32_t* const* ids, const uint8_t* const* rev,
                           const int64_t* S, const double* totals, double* const* scores_out, int32_t* const* best_out)
{
    if (n_jobs < 1 || !ctxs || !ids || !rev || !S || !totals || !scores_out || !best_out) return fail(HICMI_EINVAL, "bad arguments");
    const int NB = SUP_BASE_SLABS;
    int max_S = 1, max_n = 1;
    TableOps<SupRec> ops;
    ops.max_S = SUP_MAX_S; ops.recs = &hicmi_ctx::d_sup_recs;
    ops.size = [&](int64_t j, int64_t& n_table, int64_t& scratch, int64_t& n_rec) {
        n_table = 2 * S[j] * S[j]; scratch = S[j] * (NB + ctxs[j]->n_arr + 2 * S[j]); n_rec = S[j];
    };
    ops.append = [&](int64_t j, double* d_scores, int32_t* d_best, std::vector<SupRec>& recs, double& algo) {
        hicmi_ctx* c = ctxs[j];
        const int64_t Sj = S[j], n = c->n_arr;
        max_S = std::max(max_S, (int)Sj);
        max_n = std::max(max_n, (int)n);
        for (int64_t k = 0; k < Sj; k++) {
            SupRec d;
            memset(&d, 0, sizeof(d));
            const int32_t sid = ids[j][k];
            d.M2 = c->dM2; d.H = c->d_H; d.ld2 = c->ld2;
            d.pos = c->d_pos2sel; d.arr_pos = c->d_arr_packed + Sj;
            d.partial = c->d_ins_partial + k * (NB + n + 2 * Sj);
            d.scores = d_scores + 2 * Sj * k; d.best = d_best + 2 * k;
            d.total = totals[j];
            d.n = (int32_t)n; d.S = (int32_t)Sj; d.j = (int32_t)k;
            d.start = c->h_scaf_start[(size_t)sid]; d.L = c->h_scaf_len[(size_t)sid]; d.cur_rev = rev[j][k] ? 1 : 0;
            recs.push_back(d);
            const double nn = (double)(n - d.L);
            algo += 8.0 * (0.5 * nn * nn + nn * nn + 2.0 * (double)Sj * (double)d.L * nn);
        }
        return (int)HICMI_OK;
    };
    ops.launch = [&](const SupRec* d_recs, int n_rec) { launch_sup(d_recs, n_rec, max_S, max_n, kNearTop, ctxs[0]->stream); };
    return run_table_jobs(n_jobs, ctxs, ids, rev, S, totals, scores_out, best_out, ops);
}

int hicmi_p2_support(hicmi_ctx* c, const int32_t* ids, const uint8_t* rev, int64_t S, double total, double* scores_out,
                     int32_t* best_out)
{
    return hicmi_p2_support_multi(1, &c, &ids, &rev, &S, &total, &scores_out, &best_out);
}

// Break support (k_part2_breaks.hip): every scaffold of every job's arrangement cut at every bin boundary, the two
// pieces swapped and / or reversed in place; one record per (job, scaffold of at least 2 bins).
int hicmi_p2_breaks_multi(int64_t n_jobs, hicmi_ctx* const* ctxs, const int32_t* const* ids, const uint8_t* const* rev,
                          const int64_t* S, const double* totals, int64_t min_piece, double* const* scores_out,
                          int32_t* const* best_out)
{
    if (n_jobs < 1 || !ctxs || !ids || !rev || !S || !totals || !scores_out || !best_out || min_piece < 1)
        return fail(HICMI_EINVAL, "bad arguments");
    const int NB = BRK_BASE_SLABS;
    int64_t n_wg = 0;
    TableOps<BrkRec> ops;
    ops.max_S = 0; ops.recs = &hicmi_ctx::d_brk_recs;
    ops.size = [&](int64_t j, int64_t& n_table, int64_t& scratch, int64_t& n_rec) {
        scratch = NB;
        for (int64_t k = 0; k < S[j]; k++) {
            const int64_t L = ctxs[j]->h_scaf_len[(size_t)ids[j][k]];
            if (L < 2) continue;
            n_table += 8 * (L - 1); scratch += L * L + 3 * (L - 1); n_rec++;
        }
    };
    ops.append = [&](int64_t j, double* d_scores, int32_t* d_best, std::vector<BrkRec>& recs, double& algo) {
        hicmi_ctx* c = ctxs[j];
        const int64_t Sj = S[j], n = c->n_arr;
        // one-bin scaffolds have no record: their (-1, 0) is written here, beside the records' pairs
        int rc = upload(ctxs[0], d_best, best_out[j], sizeof(int32_t) * (size_t)(2 * Sj));
        if (rc) return rc;
        double* scratch = c->d_ins_partial + NB;
        int64_t row = 0;
        bool first = true;
        for (int64_t k = 0; k < Sj; k++) {
            const int64_t L = c->h_scaf_len[(size_t)ids[j][k]];
            if (L < 2) continue;
            BrkRec d;
            memset(&d, 0, sizeof(d));
            d.M2 = c->dM2; d.H = c->d_H; d.ld2 = c->ld2;
            d.pos = c->d_pos2sel;
            d.X = scratch; d.pq = scratch + L * L; scratch += L * L + 3 * (L - 1);
            d.base = c->d_ins_partial;
            d.scores = d_scores + 8 * row; d.best = d_best + 2 * k; row += L - 1;
            d.total = totals[j];
            d.wg0 = n_wg;
            d.n = (int32_t)n; d.B = c->h_arr_pos[(size_t)k]; d.L = (int32_t)L;
            d.min_piece = (int32_t)std::min<int64_t>(min_piece, 1 << 30);
            d.n_base = first ? NB : 0;
            first = false;
            n_wg += d.n_base + L * ((L + 3) / 4) + (L - 1);
            recs.push_back(d);
            algo += 8.0 * ((double)L * (double)L * (double)(n - L) + (double)L * (double)L * (double)L / 6.0);
        }
        algo += 4.0 * (double)n * (double)n;
        if (n_wg > 0x7fffffff) return fail(HICMI_EUNSUPPORTED, "more than 2^31 - 1 workgroups in one call");
        return (int)HICMI_OK;
    };
    ops.launch = [&](const BrkRec* d_recs, int n_rec) { launch_brk(d_recs, n_rec, n_wg, kNearTop, ctxs[0]->stream); };
    return run_table_jobs(n_jobs, ctxs, ids, rev, S, totals, scores_out, best_out, ops);
}

int hicmi_p2_breaks(hicmi_ctx* c, const int32_t* ids, const uint8_t* rev, int64_t S, double total, int64_t min_piece,
                    double* scores_out, int32_t* best_out)
{
    return hicmi_p2_breaks_multi(1, &c, &ids, &rev, &S, &total, min_piece, &scores_out, &best_out);
}

// Inversion support (k_part2_invert.hip): the scaffolds i ... j of every job's arrangement reversed and flipped, for
// every i <= j; one record per (job, left end i).
int hicmi_p2_inversions_multi(int64_t n_jobs, hicmi_ctx* const* ctxs, const int32_t* const* ids, const uint8_t* const* rev,
                              const int64_t* S, const double* totals, int64_t max_span, double* const* scores_out,
                              int32_t* const* best_out)
{
    if (n_jobs < 1 || !ctxs || !ids || !rev || !S || !totals || !scores_out || !best_out || max_span < 0)
        return fail(HICMI_EINVAL, "bad arguments");
    const int NB = INV_BASE_SLABS;
    // the bound on a call's work; HICMI_P2_INVERT_MAX_WORK lowers or raises it (tests refuse a small job with it)
    const char* env = getenv("HICMI_P2_INVERT_MAX_WORK");
    const double max_work = env && *env ? atof(env) : INV_MAX_WORK;
    const int64_t span = std::min<int64_t>(max_span, INV_MAX_S);
    int64_t n_wg = 0;
    double work = 0.0;
    TableOps<InvRec> ops;
    ops.max_S = INV_MAX_S; ops.recs = &hicmi_ctx::d_inv_recs;
    ops.size = [&](int64_t j, int64_t& n_table, int64_t& scratch, int64_t& n_rec) {
        n_table = S[j] * S[j]; scratch = NB; n_rec = S[j];
    };
    ops.append = [&](int64_t j, double* d_scores, int32_t* d_best, std::vector<InvRec>& recs, double& algo) {
        hicmi_ctx* c = ctxs[j];
        const int64_t Sj = S[j], n = c->n_arr;
        const double work0 = work;
        for (int64_t i = 0; i < Sj; i++) {
            InvRec d;
            memset(&d, 0, sizeof(d));
            d.M2 = c->dM2; d.H = c->d_H; d.ld2 = c->ld2;
            d.pos = c->d_pos2sel; d.arr_pos = c->d_arr_packed + Sj;
            d.base = c->d_ins_partial;
            d.scores = d_scores + Sj * i; d.best = d_best + 2 * i;
            d.total = totals[j];
            d.wg0 = n_wg;
            d.n = (int32_t)n; d.S = (int32_t)Sj; d.i = (int32_t)i;
            d.n_j = (int32_t)(span > 0 ? std::min<int64_t>(Sj - i, span) : Sj - i);
            d.max_span = (int32_t)span;
            d.n_base = i == 0 ? NB : 0;
            n_wg += d.n_base + d.n_j;
            recs.push_back(d);
            for (int64_t k = i; k < i + d.n_j; k++) {
                const double len = (double)(c->h_arr_pos[(size_t)k + 1] - c->h_arr_pos[(size_t)i]);
                work += len * ((double)n - len);
            }
        }
        algo += 8.0 * (0.5 * (double)n * (double)n + (work - work0));
        if (work > max_work)
            return fail(HICMI_EUNSUPPORTED, "inversion table of %.3g matrix reads (limit %.3g): set max_span to bound the segments",
                        work, max_work);
        if (n_wg > 0x7fffffff) return fail(HICMI_EUNSUPPORTED, "more than 2^31 - 1 workgroups in one call: set max_span");
        return (int)HICMI_OK;
    };
    ops.launch = [&](const InvRec* d_recs, int n_rec) { launch_inv(d_recs, n_rec, n_wg, kNearTop, ctxs[0]->stream); };
    return run_table_jobs(n_jobs, ctxs, ids, rev, S, totals, scores_out, best_out, ops);
}

int hicmi_p2_inversions(hicmi_ctx* c, const int32_t* ids, const uint8_t* rev, int64_t S, double total, int64_t max_span,
                        double* scores_out, int32_t* best_out)
{
    return hicmi_p2_inversions_multi(1, &c, &ids, &rev, &S, &total, max_span, &scores_out, &best_out);
}

int hicmi_p2_scan_pass(hicmi_ctx* c, int32_t* ids, uint8_t* rev, int64_t S, int64_t k, double total, double* best_io,
                       double* cur_fast_io, int32_t* improved_out)
{
    // one round of scanOrdering (OG:513-541): windows first = 0 .. S-k, each applied before the next.
    // Until a window improves, all of them see the same arrangement, so they are scored in batches of
    // up to 32 windows per launch pair; after an improvement the remaining windows are scored again
    // against the new arrangement.
    if (!c || !ids || !rev || !best_io || !cur_fast_io || !improved_out || S < 1 || k < 1 || k > S)
        return fail(HICMI_EINVAL, "bad arguments");
    const int64_t n_ori = c->n_orients, n_cand = c->n_orders * c->n_orients;
    int rc = hicmi_p2_set_arrangement(c, ids, rev, S);
    if (rc) return rc;
    rc = check_window_call(c, 0, k);
    if (rc) return rc;
    *improved_out = 0;                                      // (a refused call has written nothing)
    use_total(c, total);
    const int64_t last = S - k;
    std::vector<double> delta;
    int64_t first = 0;
    // windows scored per launch pair: 8, doubling while no window improves (an improvement throws the rest of the batch
    // away); a round that follows a round with at most one improvement starts at 32 (hicmi_p2_scan_all: the late rounds
    // of a chromosome change little, and a batch costs a launch pair + a synchronisation whatever its size)
    int64_t batch = c->scan_first_batch > 0 ? c->scan_first_batch : 8;
    int64_t n_improved = 0;
    std::vector<int64_t> n_near; std::vector<std::vector<int64_t>> near; std::vector<std::vector<double>> near_fast;
    while (first <= last) {
        const int64_t count = std::min<int64_t>(batch, last - first + 1);
        // wide windows: short lists from the device (cur_fast and the floor are the same for every window of the batch,
        // which ends at the first improvement); a list beyond the cap sends the batch down the delta path
        bool on_device = k >= c->near_min_k;
        if (on_device) {
            rc = window_near_batch(c, first, count, k, total, *best_io, *cur_fast_io, kNearCap, n_near, near, near_fast);
            if (rc) return rc;
            for (int64_t w = 0; w < count; w++) on_device = on_device && n_near[(size_t)w] <= kNearCap;
        }
        if (!on_device) {
            delta.resize((size_t)(count * n_cand));
            rc = window_batch(c, first, count, k, delta.data());
            if (rc) return rc;
        }
        bool applied = false;
        for (int64_t wdx = 0; wdx < count && !applied; wdx++) {
            int64_t pick = -1; double best = *best_io, pf = *cur_fast_io;
            double cf = *cur_fast_io;
            if (on_device)
                rc = decide_from_near(c, first + wdx, k, total, *best_io, cf, window_c0(c, first + wdx, k), near[(size_t)wdx],
                                      near_fast[(size_t)wdx], &pick, &best, &pf);
            else
                rc = decide_from_delta(c, first + wdx, k, total, *best_io, cf, delta.data() + wdx * n_cand, &pick, &best, &pf);
            if (rc) return rc;
            *cur_fast_io = pf;
            if (pick < 0) continue;
            *best_io = best; *improved_out = 1;
            const int64_t f = first + wdx;
            const int8_t* ord = c->h_orders.data() + (pick / n_ori) * k;
            const uint8_t* ori = c->h_orients.data() + (pick % n_ori) * k;
            int32_t wid[8];
            for (int64_t j = 0; j < k; j++) wid[j] = ids[f + ord[j]];
            for (int64_t j = 0; j < k; j++) { ids[f + j] = wid[j]; rev[f + j] = ori[j] ? 1 : 0; }
            rc = hicmi_p2_set_arrangement(c, ids, rev, S);
            if (rc) return rc;
            first = f + 1;
            applied = true;
            n_improved++;
            batch = 8;
        }
        if (!applied) { first += count; batch = std::min<int64_t>(batch * 2, 32); }
    }
    c->scan_last_improved = n_improved;
    return HICMI_OK;
}

int hicmi_p2_scan_all(hicmi_ctx* c, int32_t* ids, uint8_t* rev, int64_t S, int64_t k, double total, double* best_io,
                      double* cur_fast_io, int64_t* rounds_out)
{
    // scanOrdering's outer loop (OG:509-547) as ONE call: a chromosome's ~20 rounds are ~20 returns to the interpreter
    // otherwise, each of which waits for the interpreter lock behind the other chromosomes' threads
    if (!rounds_out) return fail(HICMI_EINVAL, "bad arguments");
    c->scan_first_batch = 0;
    for (int64_t rounds = 0;;) {
        int32_t improved = 0;
        int rc = hicmi_p2_scan_pass(c, ids, rev, S, k, total, best_io, cur_fast_io, &improved);
        c->scan_first_batch = (rc == 0 && c->scan_last_improved <= 1) ? 32 : 0;
        if (rc || !improved) { c->scan_first_batch = 0; }
        if (rc) return rc;                                  // (refused in its first round, the call has written nothing)
        *rounds_out = ++rounds;
        if (!improved) return HICMI_OK;
        if (rounds > 100000) return fail(HICMI_ESTATE, "scanOrdering does not converge");
    }
}

int hicmi_p2_scan_arranged(hicmi_ctx* c, int32_t* ids, uint8_t* rev, int64_t S, int64_t k, const int8_t* orders,
                           int64_t n_orders, const uint8_t* orients, int64_t n_orients, double* total_out, double* best_io,
                           int64_t* rounds_out)
{
    // scanOrdering (OG:495-549) from the arrangement the insertion phase left, all of it in one call: the arrangement,
    // its total in exactly that order (OG:506), the window tables for k unless they are the loaded ones, then the rounds
    if (!c || !ids || !rev || !orders || !orients || !total_out || !best_io || !rounds_out || S < 1 || k < 1 || k > S)
        return fail(HICMI_EINVAL, "bad arguments");
    int rc = hicmi_p2_set_arrangement(c, ids, rev, S);
    if (rc) return rc;
    double total = 0.0;                                    // fewer than 2 bins: nothing above the diagonal
    if (c->n_arr >= 2) { rc = hicmi_p2_arrangement_total(c, &total); if (rc) return rc; }
    *total_out = total;
    const bool loaded = c->tab_k == (int)k && c->n_orders == n_orders && c->n_orients == n_orients
                        && (int64_t)c->h_orders.size() == n_orders * k && (int64_t)c->h_orients.size() == n_orients * k
                        && !memcmp(c->h_orders.data(), orders, (size_t)(n_orders * k))
                        && !memcmp(c->h_orients.data(), orients, (size_t)(n_orients * k));
    if (!loaded) { rc = hicmi_p2_window_tables(c, k, orders, n_orders, orients, n_orients); if (rc) return rc; }
    double cur_fast = std::nan("");
    return hicmi_p2_scan_all(c, ids, rev, S, k, total, best_io, &cur_fast, rounds_out);
}

int hicmi_p2_start_all(int64_t n_jobs, hicmi_ctx* const* ctxs, const int32_t* sel, const int64_t* n_sel,
                       const int32_t* scaf_start, const int32_t* scaf_len, const int64_t* n_scaf, const int32_t* first_ids,
                       const int64_t* k, const int8_t* const* orders, const int64_t* n_orders, const uint8_t* const* orients,
                       const int64_t* n_orients, double* total_out, int64_t* pick_out, double* cost_out, int32_t* status_out)
{
    // _startChromosome (OG:551-576 up to the brute force) of n_jobs chromosomes, one context each: what hicmi_p2_select,
    // _layout, _set_arrangement, _arrangement_total, _window_tables and _decide_window(0, k, total, 0., NaN) do for one
    // chromosome, through the same functions, but PHASE BY PHASE over all jobs - everything of a phase is queued on each
    // job's own stream before any stream is waited for, so the jobs overlap on the device and the calling thread waits
    // three times per job instead of five or six
    if (n_jobs < 1 || !ctxs || !sel || !n_sel || !scaf_start || !scaf_len || !n_scaf || !first_ids || !k || !orders || !n_orders
        || !orients || !n_orients || !total_out || !pick_out || !cost_out || !status_out)
        return fail(HICMI_EINVAL, "bad arguments");
    const size_t nj = (size_t)n_jobs;
    std::vector<int64_t> sel_off(nj), scaf_off(nj), id_off(nj);
    int64_t n_max = 0;
    {
        int64_t so = 0, fo = 0, io = 0;
        for (size_t j = 0; j < nj; j++) {
            if (int rc = check_job_context(ctxs, (int64_t)j)) return rc;
            if (n_sel[j] < 1 || n_scaf[j] < 1 || k[j] < 1 || k[j] > 8 || k[j] > n_scaf[j]) return fail(HICMI_EINVAL, "bad job %lld", (long long)j);
            if (!orders[k[j]] || !orients[k[j]] || n_orders[k[j]] < 1 || n_orients[k[j]] < 1)
                return fail(HICMI_EINVAL, "no order / orientation tables for k = %lld", (long long)k[j]);
            sel_off[j] = so; scaf_off[j] = fo; id_off[j] = io;
            so += n_sel[j]; fo += n_scaf[j]; io += k[j];
            n_max = std::max(n_max, n_sel[j]);
        }
    }
    std::vector<double> H;
    harmonic_table(H, n_max);                              // the same prefix for every job
    enum { DECIDED = 0, ZERO_TOTAL = 1, NO_CANDIDATE = 2 };
    enum { IDLE, TOTAL, NEAR, DELTA, LITERAL };
    std::vector<int> phase(nj, IDLE);
    auto drain = [&](int rc) {                             // an error with work in flight: leave no stream busy
        for (size_t j = 0; j < nj; j++) (void)sync_stream(ctxs[j]);
        return rc;
    };
    int rc;
    // ---- a. selection, layout, the k largest scaffolds as the arrangement, its total
    for (size_t j = 0; j < nj; j++) {
        hicmi_ctx* c = ctxs[j];
        total_out[j] = 0.0; pick_out[j] = -1; cost_out[j] = 0.0; status_out[j] = ZERO_TOTAL;
        rc = select_enqueue(c, sel + sel_off[j], n_sel[j], &H);
        if (rc) return drain(rc);
        rc = hicmi_p2_layout(c, scaf_start + scaf_off[j], scaf_len + scaf_off[j], n_scaf[j]);
        if (rc) return drain(rc);
        const int32_t* ids = first_ids + id_off[j];
        int64_t n_bins = 0;
        for (int64_t q = 0; q < k[j]; q++) {
            if (ids[q] < 0 || ids[q] >= n_scaf[j]) return drain(fail(HICMI_EINVAL, "arrangement must list distinct scaffolds of the layout"));
            n_bins += c->h_scaf_len[(size_t)ids[q]];
        }
        if (n_bins < 2) continue;                          // one bin: total 0.0 without asking the device
        const uint8_t plus[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        rc = hicmi_p2_set_arrangement(c, ids, plus, k[j]);
        if (rc) return drain(rc);
        rc = arrangement_total_enqueue(c);
        if (rc) return drain(rc);
        phase[j] = TOTAL;
    }
    for (size_t j = 0; j < nj; j++) {
        hicmi_ctx* c = ctxs[j];
        if (sync_stream(c) != hipSuccess) return drain(fail(HICMI_EHIP, "hipStreamSynchronize failed in the start phase"));
        if (phase[j] == TOTAL) memcpy(&total_out[j], c->pin_down, sizeof(double));
    }
    // ---- b. the brute force: every order and orientation of the k scaffolds (k == S: nothing lies outside the window)
    std::vector<NearPending> np(nj);
    for (size_t j = 0; j < nj; j++) {
        hicmi_ctx* c = ctxs[j];
        if (phase[j] != TOTAL || total_out[j] == 0.0) { phase[j] = IDLE; continue; }
        const int64_t kj = k[j];
        rc = hicmi_p2_window_tables(c, kj, orders[kj], n_orders[kj], orients[kj], n_orients[kj]);
        if (rc) return drain(rc);
        rc = check_window_call(c, 0, kj);
        if (rc) return drain(rc);
        use_total(c, total_out[j]);
        if (kj >= c->near_min_k) {
            double cur_fast = std::nan("");
            rc = window_near_enqueue(c, 0, 1, kj, total_out[j], 0.0, cur_fast, kNearCap, np[j]);
            phase[j] = NEAR;
        } else {
            rc = window_batch_enqueue(c, 0, 1, kj);
            phase[j] = DELTA;
        }
        if (rc) return drain(rc);
    }
    std::vector<std::vector<int64_t>> near(nj);
    std::vector<std::vector<double>> near_fast(nj);
    for (size_t j = 0; j < nj; j++) {
        hicmi_ctx* c = ctxs[j];
        if (phase[j] == NEAR) {
            std::vector<int64_t> n_near; std::vector<std::vector<int64_t>> nr; std::vector<std::vector<double>> nf;
            rc = window_near_collect(c, np[j], n_near, nr, nf);
            if (rc) return drain(rc);
            if (n_near[0] <= kNearCap) { near[j].swap(nr[0]); near_fast[j].swap(nf[0]); phase[j] = LITERAL; continue; }
            rc = window_batch_enqueue(c, 0, 1, k[j]);      // the list overflowed: the deltas, as hicmi_p2_decide_window does
            if (rc) return drain(rc);
            phase[j] = DELTA;
        }
        if (phase[j] == DELTA) {
            if (sync_stream(c) != hipSuccess) return drain(fail(HICMI_EHIP, "hipStreamSynchronize failed in the start phase"));
            if (window_c0(c, 0, k[j]) < 0) return drain(fail(HICMI_EINVAL, "current orientation not in the orientation table"));
            const int64_t n_cand = c->n_orders * c->n_orients;
            const double* delta = reinterpret_cast<const double*>(c->pin_down.get());
            std::vector<double> fast((size_t)n_cand);
            for (int64_t i = 0; i < n_cand; i++) fast[(size_t)i] = delta[(size_t)i] / total_out[j];
            short_list(fast, 0.0, near[j]);
            near_fast[j].resize(near[j].size());
            for (size_t q = 0; q < near[j].size(); q++) near_fast[j][q] = fast[(size_t)near[j][q]];
            phase[j] = LITERAL;
        }
    }
    // ---- c. the short lists in the reference's operation order, then the first strict maximum above 0. (OG:464)
    std::vector<LiteralPending> lp(nj);
    for (size_t j = 0; j < nj; j++) {
        if (phase[j] != LITERAL) continue;
        std::vector<std::vector<int32_t>> rows;
        near_rows(ctxs[j], 0, k[j], near[j], rows);
        rc = literal_enqueue(ctxs[j], rows, total_out[j], lp[j]);
        if (rc) return drain(rc);
    }
    for (size_t j = 0; j < nj; j++) {
        if (phase[j] != LITERAL) continue;
        std::vector<double> lit;
        rc = literal_collect(ctxs[j], lp[j], lit);
        if (rc) return drain(rc);
        double pick_fast = 0.0;
        pick_first_strict_max(near[j], near_fast[j], lit, 0.0, &pick_out[j], &cost_out[j], &pick_fast);
        status_out[j] = pick_out[j] >= 0 ? DECIDED : NO_CANDIDATE;
    }
    return HICMI_OK;
}

// ---- plot support (plotContactMaps.py:15-91) --------------------------------------------------------
namespace {
int plot_prepare(hicmi_ctx* c, int kind, const int32_t* order, int64_t n_sel, int32_t** d_order_out)
{
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix set");
    if (kind < 0 || kind > 2) return fail(HICMI_EINVAL, "kind must be 0 (contacts), 1 (distance) or 2 (similarity)");
    if (n_sel < 1 || (!order && n_sel != c->n)) return fail(HICMI_EINVAL, "n_sel must be the matrix size when no order is given");
    HIPCHK(hipSetDevice(c->device));
    if (kind != 0 && !c->have_sums) { int rc = compute_sums(c); if (rc) return rc; }
    *d_order_out = nullptr;
    if (order) {
        for (int64_t i = 0; i < n_sel; i++) if (order[i] < 0 || order[i] >= c->n) return fail(HICMI_EINVAL, "order entry out of range");
        int rc = ensure(c->d_plot_order, n_sel);
        if (rc) return rc;
        rc = upload(c, c->d_plot_order, order, sizeof(int32_t) * (size_t)n_sel);
        if (rc) return rc;
        *d_order_out = c->d_plot_order;
    }
    return HICMI_OK;
}
}  // namespace

int hicmi_plot_percentiles(hicmi_ctx* c, int kind, const int32_t* order, int64_t n_sel, const double* q, int64_t n_q,
                           double* out)
{
    // numpy.percentile(a, q) (method "linear") over the n_sel x n_sel cells: virtual index (N-1)*q/100, the two
    // neighbouring order statistics selected exactly on the device, numpy's _lerp on the host
    if (!c || !q || !out || n_q < 1) return fail(HICMI_EINVAL, "bad arguments");
    for (int64_t i = 0; i < n_q; i++) if (!(q[i] >= 0.0 && q[i] <= 100.0)) return fail(HICMI_EINVAL, "percentiles must be in [0, 100]");
    int32_t* d_order = nullptr;
    int rc = plot_prepare(c, kind, order, n_sel, &d_order);
    if (rc) return rc;
    rc = ensure(c->d_plot_work, (int64_t)(plot_select_state_bytes() + plot_select_hist_bytes()));
    if (rc) return rc;
    SelectState* d_state = reinterpret_cast<SelectState*>(c->d_plot_work.get());
    unsigned int* d_hist = reinterpret_cast<unsigned int*>(c->d_plot_work + plot_select_state_bytes());
    const double N = (double)n_sel * (double)n_sel;
    const int per_batch = plot_select_max_targets() / 2;
    std::vector<unsigned char> host(plot_select_state_bytes());
    for (int64_t q0 = 0; q0 < n_q; q0 += per_batch) {
        const int nb = (int)std::min<int64_t>(per_batch, n_q - q0);
        unsigned long long ranks[8];
        double frac[4];
        for (int t = 0; t < nb; t++) {
            const double virt = (N - 1.0) * (q[q0 + t] / 100.0);        // numpy: quantile * (n - 1)
            double lo = std::floor(virt);
            if (lo > N - 1.0) lo = N - 1.0;
            const double hi = std::min(lo + 1.0, N - 1.0);
            ranks[2 * t] = (unsigned long long)lo; ranks[2 * t + 1] = (unsigned long long)hi;
            frac[t] = virt - lo;
        }
        plot_select_fill(host.data(), ranks, 2 * nb);
        rc = upload(c, d_state, host.data(), host.size());
        if (rc) return rc;
        HIPCHK(hipMemsetAsync(d_hist, 0, plot_select_hist_bytes(), c->stream));
        {
            Timed t(c, F_PLOT, 6.0 * 8.0 * N);
            launch_plot_select(c->dC, c->ldc, c->d_np, c->d_seq, kind, d_order, (int)n_sel, 2 * nb, d_state, d_hist, c->stream);
        }
        HIPCHK(hipGetLastError());
        rc = download(c, host.data(), d_state, host.size());
        if (rc) return rc;
        for (int t = 0; t < nb; t++) {
            const double a = plot_select_value(host.data(), 2 * t), b = plot_select_value(host.data(), 2 * t + 1), g = frac[t];
            const double diff = b - a;                                  // numpy.lib._function_base_impl._lerp
            double v = a + diff * g;
            if (g >= 0.5) v = b - diff * (1.0 - g);
            if (diff == 0.0) v = a;
            out[q0 + t] = v;
        }
    }
    return HICMI_OK;
}

int hicmi_plot_downsample(hicmi_ctx* c, int kind, const int32_t* order, int64_t n_sel, int64_t px, double* out)
{
    if (!c || !out || px < 1 || px > n_sel) return fail(HICMI_EINVAL, "bad arguments (1 <= px <= n_sel)");
    int32_t* d_order = nullptr;
    int rc = plot_prepare(c, kind, order, n_sel, &d_order);
    if (rc) return rc;
    rc = ensure(c->d_plot_img, px * px);
    if (rc) return rc;
    {
        Timed t(c, F_PLOT, 8.0 * (double)n_sel * (double)n_sel);
        launch_plot_downsample(c->dC, c->ldc, c->d_np, c->d_seq, kind, d_order, (int)n_sel, (int)px, c->d_plot_img, c->stream);
    }
    HIPCHK(hipGetLastError());
    return download(c, out, c->d_plot_img, sizeof(double) * (size_t)(px * px));
}


// ---------------------------------------------------------------------------------------------------
// HMM boundary finder (S2C:730-942, hmm = True): hmmlearn GaussianHMM(n_components=2, covariance_type="diag") restated
// on the device, k_hmm.hip.
namespace {

// the small buffer: params | sums (4 D) | centers (2 D) | scalar slots (16)
inline double* hmm_params(hicmi_ctx* c) { return c->d_hsmall; }
inline double* hmm_sums(hicmi_ctx* c) { return c->d_hsmall + HMM_P_SCALARS * c->hmm_ld + HMM_S_COUNT; }
inline double* hmm_cen(hicmi_ctx* c) { return hmm_sums(c) + 4 * c->hmm_ld; }
inline double* hmm_slots(hicmi_ctx* c) { return hmm_cen(c) + 2 * c->hmm_ld; }

// work areas for an X of T rows and leading dimension ld (sized when a slot is built: nothing is allocated inside the
// k-means or EM loops); ensure() only grows them, so they fit every slot built before
int hmm_size_work(hicmi_ctx* c, int64_t T, int64_t ld)
{
    int rc = ensure(c->d_hwork, 10 * T);
    if (!rc) rc = ensure(c->d_hlab, 3 * T);
    if (!rc) rc = ensure(c->d_hbt, T);
    // a column pass over width D <= ld has at most min(T, 1024) and at most 2048 / ceil(D / 256) + 1 row chunks
    const int64_t cb = (ld + 255) / 256;
    const int64_t part = 4 * std::min(std::min(T, (int64_t)1024) * ld, (2048 + cb) * 256);
    if (!rc) rc = ensure(c->d_hpart, part);
    if (!rc) rc = ensure(c->d_hsmall, (HMM_P_SCALARS + 6) * ld + HMM_S_COUNT + 16);
    if (!rc) rc = ensure(c->d_hst, 4);
    return rc;
}

// the single-problem entry points work on slot s from now on
void hmm_select(hicmi_ctx* c, int s)
{
    const auto& sl = c->hslot[s];
    c->hcur = s;
    c->d_hx = sl.d_x; c->hmm_T = sl.T; c->hmm_ld = sl.ld; c->hmm_D = sl.D;
}

// (re)size slot s for a T x ld matrix; the slot is left empty (T = 0) if that fails
int hmm_slot_alloc(hicmi_ctx* c, int s, int64_t T, int64_t ld)
{
    auto& sl = c->hslot[s];
    sl.T = sl.ld = sl.D = 0;
    int rc = ensure(sl.d_x, T * ld);
    if (!rc) rc = hmm_size_work(c, T, ld);
    if (rc) { if (c->hcur == s) hmm_select(c, s); return rc; }
    sl.T = T; sl.ld = ld; sl.D = ld;
    if (c->hcur == s) hmm_select(c, s);
    return HICMI_OK;
}

int hmm_check(hicmi_ctx* c)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (c->hmm_T <= 0 || c->hmm_D <= 0) return fail(HICMI_EINVAL, "no HMM observations (hicmi_hmm_load_obs / hicmi_hmm_set_obs)");
    return HICMI_OK;
}

// model parameters in, emission operands / log transition matrix computed on the device
int hmm_upload_params(hicmi_ctx* c, const double* startprob, const double* means, const double* covars,
                      const double* transmat)
{
    const int64_t D = c->hmm_D;
    double* P = hmm_params(c);
    int rc = upload(c, P + HMM_P_MEAN * D, means, sizeof(double) * 2 * D);
    if (!rc) rc = upload(c, P + HMM_P_VAR * D, covars, sizeof(double) * 2 * D);
    double sc[HMM_S_COUNT] = {0};
    for (int q = 0; q < 4; q++) sc[HMM_S_A + q] = transmat[q];
    sc[HMM_S_PI] = startprob[0]; sc[HMM_S_PI + 1] = startprob[1];
    if (!rc) rc = upload(c, P + HMM_P_SCALARS * D, sc, sizeof(sc));
    if (rc) return rc;
    launch_hmm_params(nullptr, (int)D, 0, P, c->stream);
    HIPCHK(hipGetLastError());
    return HICMI_OK;
}

}  // namespace

int hicmi_hmm_load_obs_slot(hicmi_ctx* c, int64_t slot, const int32_t* order, int64_t n, int64_t cut, int64_t prev)
{
    if (!c || !order) return fail(HICMI_EINVAL, "bad arguments");
    if (slot < 0 || slot >= HICMI_HMM_MAX_SLOTS) return fail(HICMI_EINVAL, "slot %lld outside [0, %d)", (long long)slot, HICMI_HMM_MAX_SLOTS);
    if (!c->dC || n != c->n) return fail(HICMI_EINVAL, "order must have n entries (n = %lld)", (long long)c->n);
    if (!c->have_sums) return fail(HICMI_EINVAL, "hicmi_row_sums has not run");
    if (cut < 0 || cut >= n || prev <= cut || prev > n) return fail(HICMI_EINVAL, "need 0 <= c < p <= n");
    for (int64_t i = 0; i < n; i++)
        if (order[i] < 0 || order[i] >= n) return fail(HICMI_EINVAL, "order entry out of range");
    HIPCHK(hipSetDevice(c->device));
    const int64_t T = n - cut, D = prev - cut;
    int rc = ensure(c->d_horder, n);
    if (!rc) rc = hmm_slot_alloc(c, (int)slot, T, D);
    if (!rc) rc = upload(c, c->d_horder, order, sizeof(int32_t) * (size_t)n);
    if (rc) return rc;
    launch_hmm_obs(c->dC, c->ldc, c->d_horder, c->d_np, c->d_seq, (int)cut, (int)T, (int)D, c->hslot[slot].d_x, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_hmm_use_obs(hicmi_ctx* c, int64_t slot)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (slot < 0 || slot >= HICMI_HMM_MAX_SLOTS) return fail(HICMI_EINVAL, "slot %lld outside [0, %d)", (long long)slot, HICMI_HMM_MAX_SLOTS);
    if (c->hslot[slot].T <= 0) return fail(HICMI_EINVAL, "HMM slot %lld holds no observations", (long long)slot);
    hmm_select(c, (int)slot);
    return HICMI_OK;
}

int hicmi_hmm_load_obs(hicmi_ctx* c, const int32_t* order, int64_t n, int64_t cut, int64_t prev)
{
    int rc = hicmi_hmm_load_obs_slot(c, 0, order, n, cut, prev);
    if (!rc) hmm_select(c, 0);
    return rc;
}

int hicmi_hmm_set_obs(hicmi_ctx* c, const double* X, int64_t T, int64_t D)
{
    if (!c || !X || T < 1 || D < 1 || T > (1 << 24) || T * D > ((int64_t)1 << 31)) return fail(HICMI_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    int rc = hmm_slot_alloc(c, 0, T, D);
    if (!rc) rc = upload(c, c->hslot[0].d_x, X, sizeof(double) * (size_t)(T * D));
    if (rc) return rc;
    hmm_select(c, 0);
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_hmm_set_width(hicmi_ctx* c, int64_t D)
{
    int rc = hmm_check(c);
    if (rc) return rc;
    if (D < 1 || D > c->hmm_ld) return fail(HICMI_EINVAL, "width %lld outside [1, %lld]", (long long)D, (long long)c->hmm_ld);
    c->hmm_D = D;
    c->hslot[c->hcur].D = D;
    return HICMI_OK;
}

int hicmi_hmm_get_obs(hicmi_ctx* c, int64_t row0, int64_t nrows, double* out)
{
    int rc = hmm_check(c);
    if (rc) return rc;
    if (!out || row0 < 0 || nrows < 0 || row0 + nrows > c->hmm_T) return fail(HICMI_EINVAL, "rows out of range");
    HIPCHK(hipSetDevice(c->device));
    const int64_t ld = c->hmm_ld, D = c->hmm_D;
    if (D == ld) return download(c, out, c->d_hx + row0 * ld, sizeof(double) * (size_t)(nrows * ld));
    std::vector<double> tmp((size_t)(nrows * ld));
    rc = download(c, tmp.data(), c->d_hx + row0 * ld, sizeof(double) * tmp.size());
    if (rc) return rc;
    for (int64_t r = 0; r < nrows; r++) memcpy(out + r * D, tmp.data() + r * ld, sizeof(double) * (size_t)D);
    return HICMI_OK;
}

int hicmi_hmm_dist2(hicmi_ctx* c, const int64_t* rows, int64_t k, double* out)
{
    int rc = hmm_check(c);
    if (rc) return rc;
    if (!rows || !out || k < 1 || k > 2) return fail(HICMI_EINVAL, "k must be 1 or 2");
    for (int64_t j = 0; j < k; j++)
        if (rows[j] < 0 || rows[j] >= c->hmm_T) return fail(HICMI_EINVAL, "row out of range");
    HIPCHK(hipSetDevice(c->device));
    const int64_t T = c->hmm_T, D = c->hmm_D, ld = c->hmm_ld;
    double* cen = hmm_cen(c);
    for (int64_t j = 0; j < k; j++)
        HIPCHK(hipMemcpyAsync(cen + j * D, c->d_hx + rows[j] * ld, sizeof(double) * (size_t)D, hipMemcpyDeviceToDevice, c->stream));
    double* dist = c->d_hwork + 8 * T;
    launch_hmm_dist2(c->d_hx, ld, (int)T, (int)D, cen, (int)k, dist, c->stream);
    HIPCHK(hipGetLastError());
    return download(c, out, dist, sizeof(double) * (size_t)(k * T));
}

int hicmi_hmm_col_stats(hicmi_ctx* c, double* mean_out, double* m2_out)
{
    int rc = hmm_check(c);
    if (rc) return rc;
    if (!mean_out || !m2_out) return fail(HICMI_EINVAL, "NULL output");
    HIPCHK(hipSetDevice(c->device));
    const int64_t T = c->hmm_T, D = c->hmm_D, ld = c->hmm_ld;
    double* sums = hmm_sums(c);
    launch_hmm_colsum(0, c->d_hx, ld, (int)T, (int)D, nullptr, nullptr, nullptr, c->d_hpart, sums, c->stream);
    HIPCHK(hipGetLastError());
    rc = download(c, mean_out, sums, sizeof(double) * (size_t)D);
    if (rc) return rc;
    for (int64_t d = 0; d < D; d++) mean_out[d] /= (double)T;
    double* cen = hmm_cen(c);
    rc = upload(c, cen, mean_out, sizeof(double) * (size_t)D);
    if (rc) return rc;
    launch_hmm_colsum(0, c->d_hx, ld, (int)T, (int)D, cen, nullptr, nullptr, c->d_hpart, sums, c->stream);
    HIPCHK(hipGetLastError());
    return download(c, m2_out, sums + D, sizeof(double) * (size_t)D);
}

int hicmi_hmm_kmeans(hicmi_ctx* c, const double* centers_in, int64_t max_iter, double tol, double* centers_out,
                     int32_t* labels_out, double* inertia_out, int64_t* n_iter_out)
{
    int rc = hmm_check(c);
    if (rc) return rc;
    if (!centers_in || !centers_out || max_iter < 1) return fail(HICMI_EINVAL, "bad arguments");
    if (c->hmm_T < 2) return fail(HICMI_EINVAL, "k-means with 2 clusters needs at least 2 rows");
    HIPCHK(hipSetDevice(c->device));
    const int64_t T = c->hmm_T, D = c->hmm_D, ld = c->hmm_ld;
    double* cen = hmm_cen(c);
    double* sums = hmm_sums(c);
    double* slots = hmm_slots(c);
    double* mind = c->d_hwork + 8 * T;
    int32_t* lab[2] = {c->d_hlab, c->d_hlab + T};
    rc = upload(c, cen, centers_in, sizeof(double) * (size_t)(2 * D));
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(lab[0], 0xff, sizeof(int32_t) * (size_t)T, c->stream));     // "no label yet" (-1)
    // sklearn _kmeans_single_lloyd: labels from the current centers, new centers from those labels; stop when the labels
    // did not change (strict convergence) or the squared center shift is <= tol
    int cur = 0;                                      // lab[cur]: the latest labels
    bool strict = false;
    int64_t it = 0;
    for (it = 0; it < max_iter; it++) {
        const int nxt = cur ^ 1;
        HIPCHK(hipMemsetAsync(c->d_hst, 0, sizeof(int) * 4, c->stream));
        launch_hmm_assign(c->d_hx, ld, (int)T, (int)D, cen, lab[cur], lab[nxt], mind, c->d_hst, c->stream);
        launch_hmm_colsum(1, c->d_hx, ld, (int)T, (int)D, nullptr, lab[nxt], nullptr, c->d_hpart, sums, c->stream);
        launch_hmm_center_update(sums, (int)T, (int)D, c->d_hst, cen, slots, c->stream);
        HIPCHK(hipGetLastError());
        cur = nxt;
        double st[4];
        rc = download(c, st, slots, sizeof(st));
        if (rc) return rc;
        if (st[2] == 0.0) { strict = true; it++; break; }
        if (st[0] <= tol) { it++; break; }
    }
    if (!strict) {                                    // final labels from the final centers
        const int nxt = cur ^ 1;
        launch_hmm_assign(c->d_hx, ld, (int)T, (int)D, cen, lab[cur], lab[nxt], mind, c->d_hst, c->stream);
        HIPCHK(hipGetLastError());
        cur = nxt;
    }
    launch_hmm_sum(mind, (int)T, slots + 4, c->stream);
    HIPCHK(hipGetLastError());
    if (labels_out) { rc = download(c, labels_out, lab[cur], sizeof(int32_t) * (size_t)T); if (rc) return rc; }
    if (inertia_out) { rc = download(c, inertia_out, slots + 4, sizeof(double)); if (rc) return rc; }
    if (n_iter_out) *n_iter_out = it;
    return download(c, centers_out, cen, sizeof(double) * (size_t)(2 * D));
}

int hicmi_hmm_fit(hicmi_ctx* c, const double* startprob, double* means, double* covars, double* transmat, int64_t n_iter,
                  double tol, double* logprob_out, int64_t* n_done_out)
{
    int rc = hmm_check(c);
    if (rc) return rc;
    if (!startprob || !means || !covars || !transmat || !logprob_out || !n_done_out || n_iter < 1)
        return fail(HICMI_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    const int64_t T = c->hmm_T, D = c->hmm_D, ld = c->hmm_ld;
    rc = ensure(c->d_hhist, n_iter);
    if (!rc) rc = hmm_upload_params(c, startprob, means, covars, transmat);
    if (rc) return rc;
    double* P = hmm_params(c);
    double* sums = hmm_sums(c);
    double *L = c->d_hwork, *alpha = L + 2 * T, *beta = L + 4 * T, *gam = L + 6 * T;
    // hmmlearn BaseHMM.fit: E-step with the current parameters (its logprob is the monitor's value), M-step, then
    // the convergence test history[-1] - history[-2] < tol
    int64_t it = 0;
    double prev = 0.0;
    for (it = 0; it < n_iter; it++) {
        launch_hmm_emission(c->d_hx, ld, (int)T, (int)D, P, L, c->stream);
        launch_hmm_fb(L, (int)T, P, (int)D, alpha, beta, gam, c->d_hhist, (int)it, c->stream);
        launch_hmm_colsum(2, c->d_hx, ld, (int)T, (int)D, nullptr, nullptr, gam, c->d_hpart, sums, c->stream);
        launch_hmm_params(sums, (int)D, 1, P, c->stream);
        HIPCHK(hipGetLastError());
        double lp = 0.0;
        rc = download(c, &lp, c->d_hhist + it, sizeof(double));
        if (rc) return rc;
        logprob_out[it] = lp;
        if (it >= 1 && lp - prev < tol) { it++; break; }
        prev = lp;
    }
    *n_done_out = it;
    rc = download(c, means, P + HMM_P_MEAN * D, sizeof(double) * (size_t)(2 * D));
    if (!rc) rc = download(c, covars, P + HMM_P_VAR * D, sizeof(double) * (size_t)(2 * D));
    double sc[HMM_S_COUNT];
    if (!rc) rc = download(c, sc, P + HMM_P_SCALARS * D, sizeof(sc));
    if (rc) return rc;
    for (int q = 0; q < 4; q++) transmat[q] = sc[HMM_S_A + q];
    return HICMI_OK;
}

int hicmi_hmm_decode(hicmi_ctx* c, const double* startprob, const double* means, const double* covars,
                     const double* transmat, int32_t* states_out)
{
    int rc = hmm_check(c);
    if (rc) return rc;
    if (!startprob || !means || !covars || !transmat || !states_out) return fail(HICMI_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    const int64_t T = c->hmm_T, D = c->hmm_D, ld = c->hmm_ld;
    rc = hmm_upload_params(c, startprob, means, covars, transmat);
    if (rc) return rc;
    double* P = hmm_params(c);
    double* L = c->d_hwork;
    int32_t* states = c->d_hlab + 2 * T;
    launch_hmm_emission(c->d_hx, ld, (int)T, (int)D, P, L, c->stream);
    launch_hmm_viterbi(L, (int)T, P, (int)D, c->d_hbt, states, c->stream);
    HIPCHK(hipGetLastError());
    return download(c, states_out, states, sizeof(int32_t) * (size_t)T);
}


namespace {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The problem table and work areas of a *_multi call in d_hmulti: problems | states | done counter | centers | sums |
// column partials | out | labels.  Checks every problem, fills `pr` (device pointers included) and returns the largest
// row count, column-pass work item count and 2 D in `mx`.
int hmm_multi_plan(hicmi_ctx* c, int64_t n_prob, const int64_t* slots, const int64_t* widths, const int64_t* nrows,
                   const int64_t* rows, bool kmeans, std::vector<HmmKmProb>& pr, int64_t mx[3])
{
    if (n_prob < 1 || n_prob > HICMI_HMM_MAX_PROBLEMS)
        return fail(HICMI_EINVAL, "%lld problems outside [1, %d]", (long long)n_prob, HICMI_HMM_MAX_PROBLEMS);
    if (!slots || !widths || !rows) return fail(HICMI_EINVAL, "bad arguments");
    pr.assign((size_t)n_prob, HmmKmProb{});
    int64_t n_dbl = 0, n_lab = 0;
    mx[0] = mx[1] = mx[2] = 0;
    for (int64_t p = 0; p < n_prob; p++) {
        if (slots[p] < 0 || slots[p] >= HICMI_HMM_MAX_SLOTS || c->hslot[slots[p]].T <= 0)
            return fail(HICMI_EINVAL, "problem %lld: slot %lld holds no observations", (long long)p, (long long)slots[p]);
        const auto& sl = c->hslot[slots[p]];
        const int64_t T = sl.T, D = widths[p];
        if (D < 1 || D > sl.ld) return fail(HICMI_EINVAL, "problem %lld: width %lld outside [1, %lld]", (long long)p, (long long)D, (long long)sl.ld);
        const int nc = kmeans ? 2 : (int)nrows[p];
        if (nc < 1 || nc > 2) return fail(HICMI_EINVAL, "problem %lld: 1 or 2 rows", (long long)p);
        if (kmeans && T < 2) return fail(HICMI_EINVAL, "problem %lld: k-means with 2 clusters needs at least 2 rows", (long long)p);
        HmmKmProb& q = pr[(size_t)p];
        for (int k = 0; k < nc; k++) {
            if (rows[2 * p + k] < 0 || rows[2 * p + k] >= T) return fail(HICMI_EINVAL, "problem %lld: row out of range", (long long)p);
            q.rows[k] = rows[2 * p + k];
        }
        q.X = sl.d_x; q.ld = sl.ld; q.T = (int)T; q.D = (int)D; q.nc = nc;
        hmm_col_shape((int)T, hmm_col_chunks((int)T, (int)D), q.rows_per, q.Rr);
        n_dbl += 4 * D + (kmeans ? (int64_t)q.Rr * 2 * D : 0) + nc * T;
        n_lab += kmeans ? 2 * T : 0;
        mx[0] = std::max(mx[0], T);
        mx[1] = std::max(mx[1], (int64_t)q.Rr * ((D + 255) / 256));
        mx[2] = std::max(mx[2], 2 * D);
    }
    const size_t b_pr = align256(sizeof(HmmKmProb) * (size_t)n_prob), b_st = align256(sizeof(HmmKmState) * (size_t)n_prob);
    const size_t bytes = b_pr + b_st + 256 + sizeof(double) * (size_t)n_dbl + sizeof(int32_t) * (size_t)n_lab;
    int rc = ensure(c->d_hmulti, (int64_t)bytes);
    if (rc) return rc;
    double* dp = (double*)(c->d_hmulti + b_pr + b_st + 256);
    for (auto& q : pr) { q.cen = dp; dp += 2 * q.D; }                   // the centers of all problems are contiguous
    for (auto& q : pr) { q.sums = dp; dp += 2 * q.D; }
    if (kmeans) for (auto& q : pr) { q.part = dp; dp += (int64_t)q.Rr * 2 * q.D; }
    for (auto& q : pr) { q.out = dp; dp += (int64_t)q.nc * q.T; }       // the distances of all problems are contiguous
    int32_t* lp = (int32_t*)dp;
    if (kmeans) for (auto& q : pr) { q.lab = lp; lp += 2 * (int64_t)q.T; }
    return HICMI_OK;
}

inline HmmKmProb* hmm_multi_probs(hicmi_ctx* c) { return reinterpret_cast<HmmKmProb*>(c->d_hmulti.get()); }
inline HmmKmState* hmm_multi_states(hicmi_ctx* c, int64_t n_prob)
{
    return (HmmKmState*)(c->d_hmulti + align256(sizeof(HmmKmProb) * (size_t)n_prob));
}
inline int* hmm_multi_done(hicmi_ctx* c, int64_t n_prob)
{
    return (int*)((unsigned char*)hmm_multi_states(c, n_prob) + align256(sizeof(HmmKmState) * (size_t)n_prob));
}

}  // namespace

int hicmi_hmm_dist2_multi(hicmi_ctx* c, int64_t n_prob, const int64_t* slots, const int64_t* widths, const int64_t* nrows,
                          const int64_t* rows, double* out)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (!nrows || !out) return fail(HICMI_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    std::vector<HmmKmProb> pr;
    int64_t mx[3];
    int rc = hmm_multi_plan(c, n_prob, slots, widths, nrows, rows, false, pr, mx);
    if (!rc) rc = upload(c, hmm_multi_probs(c), pr.data(), sizeof(HmmKmProb) * pr.size());
    if (rc) return rc;
    launch_hmm_multi_seed(hmm_multi_probs(c), hmm_multi_states(c, n_prob), (int)n_prob, 2 * (int)mx[2], 0, c->stream);
    launch_hmm_dist2_multi(hmm_multi_probs(c), (int)n_prob, (int)mx[0], c->stream);
    HIPCHK(hipGetLastError());
    int64_t total = 0;
    for (const auto& q : pr) total += (int64_t)q.nc * q.T;
    return download(c, out, pr[0].out, sizeof(double) * (size_t)total);
}

int hicmi_hmm_kmeans_multi(hicmi_ctx* c, int64_t n_prob, const int64_t* slots, const int64_t* widths, const int64_t* rows,
                           const int64_t* max_iter, const double* tol, double* centers_out, double* inertia_out,
                           int64_t* n_iter_out)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (!max_iter || !tol || !centers_out || !inertia_out || !n_iter_out) return fail(HICMI_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    std::vector<HmmKmProb> pr;
    int64_t mx[3];
    int rc = hmm_multi_plan(c, n_prob, slots, widths, nullptr, rows, true, pr, mx);
    if (rc) return rc;
    int64_t steps = 0;                                         // a problem is done after at most max_iter + 1 steps
    for (int64_t p = 0; p < n_prob; p++) {
        if (max_iter[p] < 1 || max_iter[p] > (1 << 30)) return fail(HICMI_EINVAL, "problem %lld: max_iter < 1", (long long)p);
        pr[(size_t)p].max_iter = (int)max_iter[p];
        pr[(size_t)p].tol = tol[p];
        steps = std::max(steps, max_iter[p] + 1);
    }
    HmmKmProb* dpr = hmm_multi_probs(c);
    HmmKmState* dst = hmm_multi_states(c, n_prob);
    int* done = hmm_multi_done(c, n_prob);
    rc = upload(c, dpr, pr.data(), sizeof(HmmKmProb) * pr.size());
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(done, 0, sizeof(int), c->stream));
    launch_hmm_multi_seed(dpr, dst, (int)n_prob, std::max(2 * (int)mx[2], (int)mx[0]), 1, c->stream);
    HIPCHK(hipGetLastError());
    // the done count is read back every `poll` steps; a step is a no-op for a finished problem, so the interval changes
    // no result
    const char* ev = getenv("HICMI_HMM_POLL");
    const int64_t poll = ev && atoi(ev) > 0 ? atoi(ev) : 8;
    int n_done = 0;
    for (int64_t step = 0; step < steps && n_done < n_prob;) {
        for (int64_t j = 0; j < poll && step < steps; j++, step++)
            launch_hmm_kmeans_multi_step(dpr, dst, done, (int)n_prob, (int)mx[0], (int)mx[1], (int)mx[2], c->stream);
        HIPCHK(hipGetLastError());
        rc = download(c, &n_done, done, sizeof(int));
        if (rc) return rc;
    }
    if (n_done != n_prob) return fail(HICMI_ESTATE, "k-means: %d of %lld problems finished", n_done, (long long)n_prob);
    std::vector<HmmKmState> st((size_t)n_prob);
    rc = download(c, st.data(), dst, sizeof(HmmKmState) * st.size());
    if (rc) return rc;
    int64_t total = 0;
    for (int64_t p = 0; p < n_prob; p++) {
        inertia_out[p] = st[(size_t)p].inertia;
        n_iter_out[p] = st[(size_t)p].it;
        total += 2 * (int64_t)pr[(size_t)p].D;
    }
    return download(c, centers_out, pr[0].cen, sizeof(double) * (size_t)total);
}

// ---------------------------------------------------------------------------------------------------
// Louvain tail (S2C:239-349, modularity > 0): level 0 of modularity.best_partition on the device, k_louvain.hip.
namespace {

inline double* lv_diag(hicmi_ctx* c) { return c->d_lvvec; }
inline double* lv_gdeg(hicmi_ctx* c) { return c->d_lvvec + 2 * c->lv_m; }
inline double* lv_total(hicmi_ctx* c) { return c->d_lvvec + 3 * c->lv_m + 1; }

int lv_check(hicmi_ctx* c)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    if (c->lv_m <= 0) return fail(HICMI_EINVAL, "no Louvain graph (hicmi_louvain_graph / hicmi_louvain_set_graph)");
    return HICMI_OK;
}

int lv_size(hicmi_ctx* c, int64_t m)
{
    if (m < 1) return fail(HICMI_EINVAL, "the graph needs at least one node");
    if (m > LOUVAIN_MAX_M) return fail(HICMI_EUNSUPPORTED, "m = %lld > %d Louvain nodes", (long long)m, LOUVAIN_MAX_M);
    const int64_t chunks = (m * m + 8191) / 8192;
    int rc = ensure(c->d_lvA, m * m);
    if (!rc) rc = ensure(c->d_lvvec, 3 * m + 2 + chunks);
    return rc;
}

// the _Status vectors of the graph now in d_lvA.  Layout of d_lvvec: diag | row sums | gdegrees | diag.sum() | total |
// chunk sums
int lv_status(hicmi_ctx* c, int64_t m)
{
    c->lv_m = m;
    double* v = c->d_lvvec;
    launch_louvain_status(c->d_lvA, (int)m, v, v + m, v + 3 * m + 2, v + 3 * m, v + 2 * m, v + 3 * m + 1, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int lv_work(hicmi_ctx* c, size_t bytes) { return ensure(c->d_lvwork, (int64_t)bytes); }

inline size_t lv_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

int hicmi_louvain_graph(hicmi_ctx* c, const int32_t* rows, int64_t m)
{
    if (m > LOUVAIN_MAX_M) return fail(HICMI_EUNSUPPORTED, "m = %lld > %d Louvain nodes", (long long)m, LOUVAIN_MAX_M);
    if (!c || !rows) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->dC) return fail(HICMI_EINVAL, "no contact matrix");
    if (!c->have_sums) return fail(HICMI_EINVAL, "hicmi_row_sums has not run");
    if (m > c->n) return fail(HICMI_EINVAL, "m = %lld > n = %lld", (long long)m, (long long)c->n);
    for (int64_t i = 0; i < m; i++)
        if (rows[i] < 0 || rows[i] >= c->n) return fail(HICMI_EINVAL, "row entry out of range");
    c->lv_m = 0;
    int rc = lv_size(c, m);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = ensure(c->d_lvrows, m);
    if (!rc) rc = upload(c, c->d_lvrows, rows, sizeof(int32_t) * (size_t)m);
    if (rc) return rc;
    launch_louvain_graph(c->dC, c->ldc, c->d_lvrows, c->d_np, c->d_seq, (int)m, c->d_lvA, c->stream);
    HIPCHK(hipGetLastError());
    return lv_status(c, m);
}

int hicmi_louvain_set_graph(hicmi_ctx* c, const double* A, int64_t m)
{
    if (m > LOUVAIN_MAX_M) return fail(HICMI_EUNSUPPORTED, "m = %lld > %d Louvain nodes", (long long)m, LOUVAIN_MAX_M);
    if (!c || !A) return fail(HICMI_EINVAL, "bad arguments");
    c->lv_m = 0;
    int rc = lv_size(c, m);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    rc = upload(c, c->d_lvA, A, sizeof(double) * (size_t)(m * m));
    if (rc) return rc;
    return lv_status(c, m);
}

int hicmi_louvain_get_graph(hicmi_ctx* c, double* out, double* gdeg_out, double* total_out)
{
    int rc = lv_check(c);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    const int64_t m = c->lv_m;
    if (out) { rc = download(c, out, c->d_lvA, sizeof(double) * (size_t)(m * m)); if (rc) return rc; }
    if (gdeg_out) { rc = download(c, gdeg_out, lv_gdeg(c), sizeof(double) * (size_t)m); if (rc) return rc; }
    if (total_out) { rc = download(c, total_out, lv_total(c), sizeof(double)); if (rc) return rc; }
    return HICMI_OK;
}

int hicmi_louvain_level0(hicmi_ctx* c, int64_t rounds, const uint64_t* states_in, int32_t* node2com_out,
                         uint64_t* states_out, int32_t* info_out, double* degrees_out, double* internals_out)
{
    int rc = lv_check(c);
    if (rc) return rc;
    if (!states_in || !node2com_out || !states_out || !info_out || !degrees_out || !internals_out)
        return fail(HICMI_EINVAL, "NULL argument");
    if (rounds < 1 || rounds > LOUVAIN_MAX_ROUNDS)
        return fail(HICMI_EINVAL, "rounds = %lld outside [1, %d]", (long long)rounds, LOUVAIN_MAX_ROUNDS);
    for (int64_t r = 0; r < rounds; r++)
        if ((states_in[6 * r + 2] & 1) == 0 || states_in[6 * r + 4] > 1 || states_in[6 * r + 5] > 0xffffffffull)
            return fail(HICMI_EINVAL, "round %lld: not a PCG64 state (odd increment, has_uint32 0/1, 32-bit uinteger)",
                        (long long)r);
    HIPCHK(hipSetDevice(c->device));
    const int64_t m = c->lv_m, R = rounds;
    const bool in_lds = louvain_round_bytes((int)m) <= (size_t)louvain_level0_lds_max();
    const size_t b_st = lv_align(sizeof(uint64_t) * 6 * R), b_n2c = lv_align(sizeof(int32_t) * R * m),
                 b_info = lv_align(sizeof(int32_t) * 4 * R), b_vec = lv_align(sizeof(double) * R * m),
                 b_scr = in_lds ? 0 : lv_align(louvain_round_bytes((int)m) * R);
    rc = lv_work(c, 2 * b_st + b_n2c + b_info + 2 * b_vec + b_scr);
    if (rc) return rc;
    unsigned char* p = c->d_lvwork;
    uint64_t* st_in = reinterpret_cast<uint64_t*>(p); p += b_st;
    uint64_t* st_out = reinterpret_cast<uint64_t*>(p); p += b_st;
    int32_t* n2c = reinterpret_cast<int32_t*>(p); p += b_n2c;
    int32_t* info = reinterpret_cast<int32_t*>(p); p += b_info;
    double* deg = reinterpret_cast<double*>(p); p += b_vec;
    double* inr = reinterpret_cast<double*>(p); p += b_vec;
    unsigned char* scratch = in_lds ? nullptr : p;
    rc = upload(c, st_in, states_in, sizeof(uint64_t) * 6 * R);
    if (rc) return rc;
    launch_louvain_level0(c->d_lvA, (int)m, lv_gdeg(c), lv_diag(c), lv_total(c), (int)R, st_in, n2c, st_out, info, deg, inr,
                          scratch, c->stream);
    HIPCHK(hipGetLastError());
    rc = download(c, node2com_out, n2c, sizeof(int32_t) * (size_t)(R * m));
    if (!rc) rc = download(c, states_out, st_out, sizeof(uint64_t) * 6 * R);
    if (!rc) rc = download(c, info_out, info, sizeof(int32_t) * 4 * R);
    if (!rc) rc = download(c, degrees_out, deg, sizeof(double) * (size_t)(R * m));
    if (!rc) rc = download(c, internals_out, inr, sizeof(double) * (size_t)(R * m));
    return rc;
}

int hicmi_louvain_induced(hicmi_ctx* c, const int32_t* part, int64_t n_part, int64_t k, double* out)
{
    int rc = lv_check(c);
    if (rc) return rc;
    const int64_t m = c->lv_m;
    if (n_part != m) return fail(HICMI_EINVAL, "partition of %lld nodes, graph of %lld", (long long)n_part, (long long)m);
    if (!part || !out || k < 1 || k > m) return fail(HICMI_EINVAL, "bad arguments (need 1 <= k <= m)");
    // members of every community in ascending node order (a counting sort of the partition)
    std::vector<int32_t> moff((size_t)k + 1, 0), members((size_t)m);
    for (int64_t i = 0; i < m; i++) {
        if (part[i] < 0 || part[i] >= k) return fail(HICMI_EINVAL, "partition label outside [0, k)");
        moff[(size_t)part[i] + 1]++;
    }
    for (int64_t b = 0; b < k; b++) moff[(size_t)b + 1] += moff[(size_t)b];
    {
        std::vector<int32_t> fill(moff.begin(), moff.end() - 1);
        for (int64_t i = 0; i < m; i++) members[(size_t)fill[(size_t)part[i]]++] = (int32_t)i;
    }
    HIPCHK(hipSetDevice(c->device));
    const size_t b_mem = lv_align(sizeof(int32_t) * m), b_off = lv_align(sizeof(int32_t) * (k + 1)),
                 b_agg = lv_align(sizeof(double) * m * k), b_B = lv_align(sizeof(double) * k * k);
    rc = lv_work(c, b_mem + b_off + b_agg + b_B);
    if (rc) return rc;
    unsigned char* p = c->d_lvwork;
    int32_t* d_mem = reinterpret_cast<int32_t*>(p); p += b_mem;
    int32_t* d_off = reinterpret_cast<int32_t*>(p); p += b_off;
    double* agg = reinterpret_cast<double*>(p); p += b_agg;
    double* B = reinterpret_cast<double*>(p);
    rc = upload(c, d_mem, members.data(), sizeof(int32_t) * (size_t)m);
    if (!rc) rc = upload(c, d_off, moff.data(), sizeof(int32_t) * (size_t)(k + 1));
    if (rc) return rc;
    launch_louvain_induced(c->d_lvA, (int)m, d_mem, d_off, (int)k, agg, B, c->stream);
    HIPCHK(hipGetLastError());
    return download(c, out, B, sizeof(double) * (size_t)(k * k));
}

int hicmi_louvain_modularity(hicmi_ctx* c, const int32_t* parts, int64_t rounds, int64_t n_part, double* q_out)
{
    int rc = lv_check(c);
    if (rc) return rc;
    const int64_t m = c->lv_m, R = rounds;
    if (n_part != m) return fail(HICMI_EINVAL, "partitions of %lld nodes, graph of %lld", (long long)n_part, (long long)m);
    if (!parts || !q_out) return fail(HICMI_EINVAL, "NULL argument");
    if (R < 1 || R > LOUVAIN_MAX_ROUNDS) return fail(HICMI_EINVAL, "rounds = %lld outside [1, %d]", (long long)R, LOUVAIN_MAX_ROUNDS);
    for (int64_t i = 0; i < R * m; i++)
        if (parts[i] < 0 || parts[i] >= m) return fail(HICMI_EINVAL, "partition label outside [0, m)");
    HIPCHK(hipSetDevice(c->device));
    const size_t b_p = lv_align(sizeof(int32_t) * R * m), b_same = lv_align(sizeof(double) * R * m),
                 b_acc = lv_align(sizeof(double) * 3 * R * m), b_q = lv_align(sizeof(double) * R);
    rc = lv_work(c, b_p + b_same + b_acc + b_q);
    if (rc) return rc;
    unsigned char* p = c->d_lvwork;
    int32_t* d_p = reinterpret_cast<int32_t*>(p); p += b_p;
    double* same = reinterpret_cast<double*>(p); p += b_same;
    double* acc = reinterpret_cast<double*>(p); p += b_acc;
    double* q = reinterpret_cast<double*>(p);
    rc = upload(c, d_p, parts, sizeof(int32_t) * (size_t)(R * m));
    if (rc) return rc;
    launch_louvain_score(c->d_lvA, (int)m, d_p, (int)R, lv_gdeg(c), lv_total(c), same, acc, q, c->stream);
    HIPCHK(hipGetLastError());
    return download(c, q_out, q, sizeof(double) * (size_t)R);
}

// ---------------------------------------------------------------------------------------------------
int hicmi_timing_reset(hicmi_ctx* c)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    int rc = resolve_timing(c);
    if (rc) return rc;
    for (int f = 0; f < F_COUNT; f++) { c->ms[f] = 0; c->launches[f] = 0; c->bytes[f] = 0; }
    c->nn_scans = c->nn_scan_cols = c->nn_cache_hits = c->nn_merges = 0; c->nn_retries = 0;
    return HICMI_OK;
}

int hicmi_timing_enable(hicmi_ctx* c, int on)
{
    if (!c) return fail(HICMI_EINVAL, "NULL context");
    int rc = resolve_timing(c);
    if (rc) return rc;
    c->timing = on < 0 ? 0 : (on > 2 ? 1 : on);
    return HICMI_OK;
}

int hicmi_timing_get(hicmi_ctx* c, char* names_out, int64_t names_cap, double* ms_out, int64_t* launches_out,
                     double* bytes_out, int64_t cap, int64_t* count_out)
{
    if (!c || !names_out || !ms_out || !launches_out || !bytes_out || !count_out) return fail(HICMI_EINVAL, "NULL argument");
    if (cap < F_COUNT) return fail(HICMI_EINVAL, "need room for %d families", (int)F_COUNT);
    int rc = resolve_timing(c);
    if (rc) return rc;
    std::string names;
    for (int f = 0; f < F_COUNT; f++) {
        if (f) names += ";";
        names += kFamilyNames[f];
        ms_out[f] = c->ms[f]; launches_out[f] = c->launches[f]; bytes_out[f] = c->bytes[f];
    }
    if ((int64_t)names.size() + 1 > names_cap) return fail(HICMI_EINVAL, "names buffer too small");
    memcpy(names_out, names.c_str(), names.size() + 1);
    *count_out = F_COUNT;
    return HICMI_OK;
}

}  // extern "C"
