/*
 * hicmi.h - C ABI of libhicmi.so: the MI355X (gfx950) hot path of Hi-C contact-map clustering
 * (Part 1) and scaffold ordering (Part 2).
 *
 * The reference (AO33/HiC_Genome_Assembler) is pure Python and has no FFI of its own
 * (SURVEY.md section 8b); the boundary a maintainer would bind is therefore defined here, one entry
 * point per native routine the reference reaches through NumPy / SciPy / Numba.  Each
 * declaration cites the reference call site it replaces (paths relative to
 * HIC_ASSEMBLER/; S2C = scaffoldToChromosomes.py, OG = orderGenome.py).  INTEGRATION.md shows
 * the ctypes stub for each.
 *
 * Conventions: every function returns 0 on success and a negative HICMI_E* code on failure;
 * hicmi_last_error() returns a message for the calling thread.  Host buffers are caller-owned,
 * plain pointers and sizes only.  A context belongs to one host thread and one GPU; all work
 * is issued on the context's own HIP stream and every call that returns host data has
 * synchronised that stream before returning.  Matrices are row-major.
 *
 * There is NO CPU fallback anywhere in this library: without a HIP device hicmi_create fails.
 */
#ifndef HICMI_H
#define HICMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HICMI_ABI_VERSION 1

#define HICMI_OK            0
#define HICMI_EINVAL       -1   /* bad argument / call order */
#define HICMI_EHIP         -2   /* HIP runtime error (message has the hipError string) */
#define HICMI_ENOMEM       -3   /* a device allocation failed, whichever call made it (message has the byte count); a
                                   failed pinned host allocation is HICMI_EHIP */
#define HICMI_ESTATE       -4   /* kernel reported an internal inconsistency (e.g. nn-chain guard) */
#define HICMI_EUNSUPPORTED -5   /* e.g. more than 65536 bins (rank matrix is uint16 in this version) */

typedef struct hicmi_ctx hicmi_ctx;

int         hicmi_abi_version(void);
const char *hicmi_last_error(void);
int         hicmi_device_count(int *count);

/* One context per GPU / per process rank. */
int hicmi_create(int device, hicmi_ctx **out);
int hicmi_destroy(hicmi_ctx *ctx);
/* The HIP stream all kernels of this context are launched on (hipStream_t as void*), so a caller
 * can bracket launches with its own events. */
int hicmi_stream(hicmi_ctx *ctx, void **stream_out);
int hicmi_synchronize(hicmi_ctx *ctx);

/* ---- contact matrix -------------------------------------------------------------------------
 * Replaces the dense fp64 matrix built by buildAdjacencyMatrix (S2C:70-98, OG:65-93).
 * _host copies n*n doubles to the GPU; _device adopts a caller-owned device allocation (leading
 * dimension ld >= n, in elements) without copying - the caller keeps it alive and unchanged.
 *
 * What a new matrix invalidates.  A context is kept over many maps, and its state falls into three classes
 * (tests/test_gpu_stale_state.py holds every call below to this rule):
 *   REPLACERS put another matrix under the context: hicmi_set_contacts_host, _host_f32, _device, hicmi_compact,
 *     hicmi_rebin, hicmi_map_finish of a plain and of a lifted build (and the file calls that end in it:
 *     hicmi_build_maps, hicmi_lift_maps, hicmi_split_maps), hicmi_ice_mask_rows, hicmi_ice_balance.
 *     hicmi_set_row_sums keeps the matrix and replaces the sums.
 *   INVALIDATED by every replacer of the matrix - the call that rebuilds it in brackets; until then every call that
 *     answers from it returns HICMI_EINVAL "<that call> has not run" and writes nothing:
 *       the computed row sums (recomputed on demand; hicmi_compact, hicmi_rebin and hicmi_map_finish recompute them);
 *       the merges of hicmi_get_raw_merges [hicmi_upgma];
 *       the rank matrix, its pre-sort and the cached row of hicmi_cut_scan: hicmi_get_rank_rows, hicmi_cut_scan,
 *         hicmi_filter_scan, hicmi_first_pass_cuts, hicmi_filter_cuts and their _multi forms, and
 *         hicmi_get_similarity_row, which reads the leaf order that call uploads [hicmi_rank_matrix];
 *       the Part 2 selection: hicmi_p2_total, _score, _score_exact, _layout [hicmi_p2_select];
 *       the layout: hicmi_p2_set_arrangement, _decide_insertion, _insert_all, _support, _breaks, _inversions, _scan_pass,
 *         _scan_all, _scan_arranged and their _multi forms [hicmi_p2_layout];
 *       the arrangement, its literal score and the cache of exact scores: hicmi_p2_arrangement_total,
 *         _arrangement_score, _score_insertions, _score_window, _decide_window, _window_shortlist
 *         [hicmi_p2_set_arrangement].
 *     hicmi_set_row_sums invalidates what depends on the sums: the merges (the distances divide by np_sum) and the rank
 *     matrix with its pre-sort and cached scan row (the similarity keys multiply by seq_sum).  Part 2 reads the matrix
 *     alone and stands.
 *   SNAPSHOTS are copies and survive every replacer bit for bit: the HMM observation slots, the Louvain graph, the
 *     window order and orientation tables of hicmi_p2_window_tables, the resident pair store with the rows of the last
 *     links call, and every build that is open between its _begin and its _finish (map, span, ends, anchor) - it
 *     finishes to the result it gives undisturbed.
 *   STATELESS calls read the matrix (and the sums) as they stand at the call and keep nothing: hicmi_row_sums,
 *     hicmi_get_contact_rows, hicmi_group_sums, hicmi_junction_sums, hicmi_plot_*,
 *     hicmi_pair_stats, hicmi_split_pairs and the *_resident calls. */
int hicmi_set_contacts_host(hicmi_ctx *ctx, const double *contacts, int64_t n);
/* The same from an fp32 host matrix (BASELINE.json configs[4]: 64,000 bins stored as fp32): half the host memory and
 * PCIe traffic; the values are widened to fp64 on the device and every stage computes on exactly those values. */
int hicmi_set_contacts_host_f32(hicmi_ctx *ctx, const float *contacts, int64_t n);
int hicmi_set_contacts_device(hicmi_ctx *ctx, const double *d_contacts, int64_t n, int64_t ld);
/* Device address, size and leading dimension of the context's contact matrix, so that further
 * contexts on the same GPU (e.g. one per chromosome worker thread in Part 2, chromosomes being
 * independent - OG:608-612) can adopt it with hicmi_set_contacts_device instead of copying it. */
int hicmi_contacts_device(hicmi_ctx *ctx, void **d_contacts_out, int64_t *n_out, int64_t *ld_out);

/* Host-side loader (no GPU involved): buildAdjacencyMatrix's triplet parse (S2C:70-98, OG:65-93).
 * `path`: HiC-Pro matrix file, lines "id1<TAB>id2<TAB>value"; bin_ids[0..n): the bin ID of every
 * row; out: n*n doubles (zero-filled here).  Triplets naming an unknown ID are skipped, each one sets
 * [i][j] and [j][i], a cell named twice keeps the later line's value, values are converted with
 * correct rounding (as Python's float()).  threads <= 0: all hardware threads.  A malformed line is
 * an error (the reference raises there).  edges_out (may be NULL): triplets used. */
int hicmi_load_hicpro_matrix(const char *path, const int64_t *bin_ids, int64_t n, double *out, int threads,
                             int64_t *edges_out);

/* Host-side writer (no GPU involved) of HiC-Pro's *_iced.matrix, the file hicmi_load_hicpro_matrix reads (replaces the
 * `%f` output of HiC-Pro's ice script; -part0): the upper triangle with the diagonal of the dense n x n matrix `mat`, row
 * then column ascending, non-zero values only, "id1<TAB>id2<TAB>value" with bin_ids[i] the ID of row i.  Values are
 * written as Python's repr(float) writes them - the shortest digits that read back to the same double - so the loader
 * gives back `mat` bit for bit.  threads <= 0: all hardware threads.  entries_out (may be NULL): lines written.
 * hicmi_format_double: that text of one value (NUL-terminated; cap >= 32), for tests. */
int hicmi_write_hicpro_matrix(const char *path, const double *mat, int64_t n, const int64_t *bin_ids, int threads,
                              int64_t *entries_out);
int hicmi_format_double(double v, char *out, int64_t cap);

/* Row sums, both flavours the reference uses:
 *   np_sum[i]  = row.sum() as NumPy reduces it (pairwise, 8192-element chunks)   S2C:112, S2C:147
 *   seq_sum[i] = builtin sum() left to right                                     S2C:134
 * Either output may be NULL.  Results are also kept on the device for the later stages. */
int hicmi_row_sums(hicmi_ctx *ctx, double *np_sum, double *seq_sum);

/* One map over several GPUs (first bullet): the row-independent stages - row sums (S2C:112,134), the
 * per-row argsort (S2C:1132) and the per-row counts of the cut and filter scans (S2C:455-459, 622-636) - are computed
 * only for the rows first, first + stride, first + 2 stride, ... of this context (a CYCLIC row partition: the scans
 * read a triangle of the rank matrix, contiguous blocks would leave the last rank with most of it).  Afterwards
 *   hicmi_row_sums      fills only the owned entries (0 elsewhere) until hicmi_set_row_sums installs the gathered vectors,
 *   hicmi_rank_matrix   sorts and inverts only the owned rows,
 *   hicmi_cut_scan / hicmi_filter_scan  return counts and flags of the owned rows, 0 for the others;
 * the caller all-gathers the owned entries across the ranks (hic_genome_assembler_amd/dist.py: RCCL through
 * torch.distributed).  first = 0, stride = 1 (the default) is the whole matrix. */
int hicmi_set_row_shard(hicmi_ctx *ctx, int64_t first, int64_t stride);
int hicmi_set_row_sums(hicmi_ctx *ctx, const double *np_sum, const double *seq_sum);

/* removeRows (S2C:100-136): keep only rows/columns keep[0..n_keep) (ascending); recomputes both
 * row sums on the compacted matrix.  The compacted copy is owned by the context (an adopted
 * device matrix is left untouched). */
int hicmi_compact(hicmi_ctx *ctx, const int32_t *keep, int64_t n_keep);

/* A coarser raw map from the resident one.  Replaces a re-run of HiC-Pro's build_matrix at k
 * times the bin size (the reference starts from HiC-Pro's files, S2C:35-98, and its README asks for "a resolution size
 * of 100-500Kb"): HiC-Pro cuts every scaffold into bins from its own start, so the bins of the coarser map are runs of
 * consecutive fine bins of one scaffold and its raw counts are sums of the fine ones.
 * group_start: m + 1 strictly ascending entries from 0 to n; coarse bin I is the fine bins [group_start[I],
 * group_start[I + 1]), at most 64 of them.  On the context's contact matrix C as it stands (uploaded, compacted, or
 * adopted with ld >= n):
 *   R[I][J] = sum of C[i][j] over i in I, j in J                      (I != J)
 *   R[I][I] = sum of C[i][j] over i <= j, both in I: the dense map holds a read pair between two different bins twice, a
 *             pair inside one bin once, and two fine bins that fall into one coarse bin turn their pairs into such pairs.
 * So the sum over the upper triangle with the diagonal - the read pairs - is the same for R and C.  Like hicmi_compact:
 * the m x m result is owned by the context (ld = m) and replaces its matrix state, both row sums are recomputed on it,
 * and an adopted source is left untouched.  R is exactly symmetric and two calls give the same bits: every sum has a
 * fixed order (the columns of J left to right, each column's rows of I top to bottom) and R[J][I] is a copy of R[I][J];
 * for integer counts below 2^53 every order is exact.  HICMI_REBIN_PLAIN=1 in the environment takes the
 * one-thread-per-cell kernel instead (the A/B), with the same bits.
 * HICMI_EINVAL: no matrix set, m < 1, m > n, group_start not from 0 to n or not strictly ascending; HICMI_EUNSUPPORTED: a
 * coarse bin of more than 64 fine bins.  After either the context is unchanged. */
int hicmi_rebin(hicmi_ctx *ctx, const int32_t *group_start, int64_t m);

/* ---- Part 1: clustering ---------------------------------------------------------------------
 * convertMatrix(distance) + squareform + scipy average + dendrogram leaf order
 * (S2C:138-155, S2C:187-208).  Z_out: (n-1) x 4 doubles in SciPy's linkage convention (may be
 * NULL); leaves_out: n int32 (dendrogram(count_sort='ascending')['leaves']). */
int hicmi_upgma(hicmi_ctx *ctx, double *Z_out, int32_t *leaves_out);

/* reorderMatrix + convertMatrix(similarity) + numpy.argsort(axis=1)[:, ::-1]
 * (S2C:157-163, S2C:149, S2C:1132) for the row/column order `order` (n int32, normally the leaves).
 * Builds, on the device, R[a][k] = column with the k-th largest similarity in row a (ties:
 * larger column index first) and its inverse rank[a][b] = position of column b in row a. */
int hicmi_rank_matrix(hicmi_ctx *ctx, const int32_t *order);
/* How the last hicmi_rank_matrix got its rows.  hicmi_upgma starts, on a second stream beside the nn-chain, a sort of
 * every row in STORAGE numbering: a row without equal similarities has the same sorted sequence under any numbering,
 * so hicmi_rank_matrix only re-addresses it by `order`; in a row that does hold equal similarities the order inside each
 * run of equal values depends on the labels, and is made afterwards by a cheaper sort of (run, label) keys.
 * Under a row shard the pre-sort covers ALL rows (the GPU is idle during the replicated chain) and only the own rows are
 * re-addressed.  *state_out: 0 = all rows sorted by hicmi_rank_matrix itself (no hicmi_upgma before it, n < 2048 or
 * HICMI_NO_PRESORT=1), 1 = pre-sorted rows used, *tied_rows_out (may be NULL) of all rows held equal similarities,
 * 2 = pre-sort discarded (only with HICMI_PRESORT_TIES=resort, the A/B mode that re-sorts tied rows in full). */
int hicmi_presort_state(hicmi_ctx *ctx, int *state_out, int64_t *tied_rows_out);
/* Copy rows [row0, row0+nrows) of R (or of its inverse when inverse != 0) to the host as uint16. */
int hicmi_get_rank_rows(hicmi_ctx *ctx, int64_t row0, int64_t nrows, int inverse, uint16_t *out);
/* Similarity values of one reordered row (S2C:149), for tests. */
int hicmi_get_similarity_row(hicmi_ctx *ctx, int64_t row, double *out);

/* ---- Part 1: hypergeometric cut scan ---------------------------------------------------------
 * find_matrix_pvalue_breakpoints inner loop (S2C:449-469) for one `start`:
 *   x[i-start] = #{ v in R[i][0 : i-start] : start <= v <= i }           for i in (start, n)
 *   sig[i-start] = 0 if hyper_geom(x, M, i-start, i-start) >= psig else 1   (NaN counts as 1)
 * and x[0] = sig[0] = 0 (S2C:448-452).  x_out / sig_out hold n-start entries; either may be NULL.
 * The counts of the last `start` are cached, so the M-rescan of S2C:473-477 costs no matrix pass. */
int hicmi_cut_scan(hicmi_ctx *ctx, int64_t start, int64_t M, double psig, int32_t *x_out, uint8_t *sig_out);

/* filter_noisy_breakpoints row tests (S2C:622-636) for one (start, c):
 *   rows ii in [start, start+n_rows):  x = #{ v in R[ii][0 : c-start] : start <= v <= c }
 *   sig = 1 if hyper_geom(x, M, c-start, c-start) < psig else 0            (NaN counts as 0) */
int hicmi_filter_scan(hicmi_ctx *ctx, int64_t start, int64_t c, int64_t n_rows, int64_t M, double psig,
                      int32_t *x_out, uint8_t *sig_out);

/* The two scan loops as a whole, with their control flow on the device: every scan's arguments come out of the previous
 * scan's flags, so driven from the host (hicmi_cut_scan / hicmi_filter_scan in a Python loop) each of the ~230 scans of
 * a 16k map pays a launch, a download and a decision on top of its few tens of microseconds of device work.  Here the
 * decisions are kernels too (k_part1_scan.hip), the host enqueues scans in batches and reads one small record per batch.
 * Not available on a row shard (the flags of every scan would have to be gathered): the per-scan calls remain for that.
 *
 * hicmi_first_pass_cuts = pre_process_all_matrix_breakpoints (S2C:513-551) with find_matrix_pvalue_breakpoints
 * (S2C:413-511) inside: min_size >= 1; stop_ind = int(n - n * min_frac), computed by the caller; psig as the caller
 * passes it (the reference passes the literal .05, S2C:535).  cuts_out: the cut indices in the order found.  m_log_out:
 * pairs (M before, M after) of every "M value (world_size) changed" event (S2C:473-483), in order - the reference
 * prints them.
 * hicmi_filter_cuts = filter_noisy_breakpoints (S2C:553-727): cuts_in ascending; cuts_out = sorted(filtered);
 * *warned_out = how many times the "maximum number of rounds" warning (S2C:592-595) was reached. */
int hicmi_first_pass_cuts(hicmi_ctx *ctx, int64_t min_size, int64_t stop_ind, double psig, int32_t *cuts_out,
                          int64_t cuts_cap, int64_t *n_cuts_out, int32_t *m_log_out, int64_t log_cap, int64_t *n_log_out);
int hicmi_filter_cuts(hicmi_ctx *ctx, const int32_t *cuts_in, int64_t n_in, double psig, int32_t *cuts_out,
                      int64_t cuts_cap, int64_t *n_out, int64_t *warned_out);

/* The same two loops for n_sets parameter sets at once, in lock step on the resident rank matrix (Part 1 parameter
 * sweeps: sweepPart1.py).  Each set's outputs are exactly those of the single-set call with that set alone.
 * 1 <= n_sets <= HICMI_SCAN_MAX_SETS, else HICMI_EINVAL (callers split larger grids).  One scan step is one count launch
 * for every live set plus one decide launch with a workgroup per set; sets that recount at the same arguments share
 * the count (counts never depend on M, min_size or psig).  HICMI_SCAN_SHARE=0 in the environment turns that off.
 * hicmi_first_pass_cuts_multi = pre_process_all_matrix_breakpoints (S2C:513-551, with S2C:413-511 inside) for set k =
 * (min_size[k], stop_ind[k]) and the one psig of the call: cuts_out + k * cuts_cap holds n_cuts_out[k] cuts,
 * m_log_out + k * 2 * log_cap holds n_log_out[k] (M before, M after) pairs.
 * hicmi_filter_cuts_multi = filter_noisy_breakpoints (S2C:553-727) for set k = (cuts_in[cand_off[k] : cand_off[k+1]],
 * psig[k]): cuts_out + k * cuts_cap holds n_out[k] kept cuts, warned_out[k] the warnings.  An empty candidate list
 * gives an empty result (the single-set call rejects it; the reference returns [] before its loops). */
#define HICMI_SCAN_MAX_SETS 64
int hicmi_first_pass_cuts_multi(hicmi_ctx *ctx, int64_t n_sets, const int64_t *min_size, const int64_t *stop_ind, double psig,
                                int32_t *cuts_out, int64_t cuts_cap, int64_t *n_cuts_out, int32_t *m_log_out, int64_t log_cap,
                                int64_t *n_log_out);
int hicmi_filter_cuts_multi(hicmi_ctx *ctx, int64_t n_sets, const int64_t *cand_off, const int32_t *cuts_in, const double *psig,
                            int32_t *cuts_out, int64_t cuts_cap, int64_t *n_out, int64_t *warned_out);

/* hyper_geom (S2C:352-368) = scipy.stats.hypergeom.sf(x-1, M, n, N); NaN for invalid arguments.
 * Host-side scalar evaluation with the same code the kernels run. */
double hicmi_hypergeom_sf(int64_t x, int64_t M, int64_t n, int64_t N);
/* The comparison the scans make with it, as the kernels evaluate it (host build of the same routine, for tests):
 * 1 if hyper_geom(x, M, n, N) < psig, 0 if >= psig, -1 if it is NaN - the tail sum stops as soon as that is settled. */
int hicmi_hypergeom_decide(int64_t x, int64_t M, int64_t n, int64_t N, double psig);

/* Host helpers that finish scipy's linkage: stable sort of raw merges by height + union-find
 * relabel, and the count-sorted leaf walk.  Exposed for tests. */
int hicmi_label_linkage(const double *Zraw, int64_t n, double *Z_out);
int hicmi_leaf_order(const double *Z, int64_t n, int32_t *leaves_out);
/* Device self test: the Lance-Williams update divides by (nx+ny) with a 3-instruction exact sequence
 * (k_nnchain.hip: div_by_small_int); this compares it with the '/' operator on `samples` random
 * (numerator, integer divisor < 2^17) pairs and returns the number of mismatches (must be 0). */
int hicmi_selftest_division(hicmi_ctx *ctx, uint64_t seed, int64_t samples, uint64_t *mismatches_out);
/* Raw merges (x, y, height, size) in nn-chain merge order from the last hicmi_upgma. */
int hicmi_get_raw_merges(hicmi_ctx *ctx, double *Zraw_out);
/* Counters of the nn-chain kernels (scipy average, S2C:197) since the last hicmi_timing_reset, 6 doubles:
 * [0] merges, [1] row scans, [2] columns those scans visited (the "sum over scans of the live columns" of the
 * algorithmic-bytes definition), [3] chain steps answered by the neighbour cache instead of a scan,
 * [4] re-runs on one workgroup after a late peer of the column-sliced kernel, [5] reserved.
 * A chain step is one pass of SciPy's inner loop (the row of the chain's top element is scanned; the pass that confirms
 * a reciprocal pair included), and every one is counted once: [1] + [3] = SciPy's steps, for every kernel with the
 * cache; the cache-less kernel (HICMI_NNCHAIN_PLAIN=1) has [1] = SciPy's steps, [2] = the columns they visit, [3] = 0.
 * The scan fused with a merge is the next step's scan.  How the steps split between [1] and [3] depends on the epoch
 * length and the kernel, not on the number of replicas. */
int hicmi_nnchain_stats(hicmi_ctx *ctx, double *out6);

/* ---- Part 2: ordering objective --------------------------------------------------------------
 * giveNewAdjMat (OG:296-308): select the sub-matrix of the context's contact matrix for the bins
 * sel[0..n) (indices into the contact matrix); later candidates index into this selection. */
int hicmi_p2_select(hicmi_ctx *ctx, const int32_t *sel, int64_t n);
/* total = sum of all entries above the diagonal of the selected sub-matrix, with the reference's
 * own rounding: Python sum over offsets 1..n-1 of numpy.trace(adjMat, offset) (OG:343,448,506). */
int hicmi_p2_total(hicmi_ctx *ctx, double *total_out);
/* costFunction_numba (OG:184-191) of n_cand candidate orders at once.  perms: n_cand x n_used
 * int32 positions into the current selection (the reference's nOrder lists, OG:347,357,460,532);
 * n_used <= selection size.  scores_out: n_cand doubles.  Identical index lists give bit-identical
 * scores. */
int hicmi_p2_score(hicmi_ctx *ctx, const int32_t *perms, int64_t n_cand, int64_t n_used, double total,
                   double *scores_out);
/* The same objective in the reference's exact operation order (numpy.trace pairwise sums per
 * offset, then the sequential cum/total/i recurrence, OG:185-191): bit-identical to the reference's
 * NumPy path.  The search compares scores that can differ by one ulp (OG:349,359,464,535), so the
 * candidates within 1e-9 of a step's best hicmi_p2_score are re-scored with this entry point and
 * the decision is taken on these values. */
int hicmi_p2_score_exact(hicmi_ctx *ctx, const int32_t *perms, int64_t n_cand, int64_t n_used, double total,
                         double *scores_out);

/* ---- Part 2: search steps with the candidates enumerated on the device -------------------------
 * The reference builds a Python index list and a gathered matrix per candidate (OG:344-365,
 * 457-466, 519-538).  Here the scaffolds of a chromosome are contiguous ranges of the current
 * selection ("layout"), the order/orientation under test is a list of (scaffold, reversed) pairs
 * ("arrangement"), and a candidate is a couple of integers.
 *
 * hicmi_p2_layout: scaffold s occupies selection positions [scaf_start[s], scaf_start[s]+scaf_len[s]),
 * bins in ascending-ID ('+') order.  Reset by hicmi_p2_select. */
int hicmi_p2_layout(hicmi_ctx *ctx, const int32_t *scaf_start, const int32_t *scaf_len, int64_t n_scaf);
/* The arrangement = scaffolds ids[0..S) left to right, rev[j] != 0 when scaffold j is laid down
 * in '-' orientation (reorderScaffList, OG:310-321). */
int hicmi_p2_set_arrangement(hicmi_ctx *ctx, const int32_t *ids, const uint8_t *rev, int64_t S);
/* Literal total (see hicmi_p2_total) of the sub-matrix in the arrangement's order - what the
 * reference computes from giveNewAdjMat's matrix at OG:343 / OG:448 / OG:506. */
int hicmi_p2_arrangement_total(hicmi_ctx *ctx, double *total_out);
/* Closed-form objective of the arrangement itself. */
int hicmi_p2_arrangement_score(hicmi_ctx *ctx, double total, double *score_out);
/* checkAllScores (OG:332-372): objective of the arrangement with scaffold new_id inserted at every
 * gap g = 0..S in both orientations; scores_out[2*g + r], r = 1 for '-'.  2*(S+1) doubles. */
int hicmi_p2_score_insertions(hicmi_ctx *ctx, int32_t new_id, double total, double *scores_out);
/* Enumeration tables for windows of k scaffolds (permutations/removeReverseDuplicates/plusMinusPerms,
 * OG:381-430): orders is n_orders x k (window-local scaffold index per slot), orients is
 * n_orients x k (1 = '-').  Candidate c = order c / n_orients, orientation c % n_orients. */
int hicmi_p2_window_tables(hicmi_ctx *ctx, int64_t k, const int8_t *orders, int64_t n_orders,
                           const uint8_t *orients, int64_t n_orients);
/* bruteForceBestScore / scanOrdering inner loops (OG:457-466, 519-538) for the window of k
 * scaffolds starting at arrangement index `first`: delta_out[c] = (objective of candidate c) * total
 * minus a term common to all candidates of this window (the pairs that lie outside it), so
 * score(c) = score(c0) + (delta[c] - delta[c0]) / total for any candidate c0 whose score is known.
 * n_orders * n_orients doubles. */
int hicmi_p2_score_window(hicmi_ctx *ctx, int64_t first, int64_t k, double *delta_out);

/* Whole decision steps (what the drop-in Part 2 calls in its inner loops): fast scores of all
 * candidates, short list within 1e-9 of the best, literal re-scoring of the short list (cached by
 * bin order under `total`), then the reference's "first strict maximum above bestCost" rule
 * (OG:349,359,464,535) - identical decisions to doing the same with the entry points above.
 *
 * Window of k scaffolds at arrangement index `first` (k == S is bruteForceBestScore).  floor is the
 * incoming bestCost; cur_fast the fast score of the current arrangement (NaN: computed here).
 * pick_out = winning candidate index or -1; best_out = its literal score (or floor);
 * pick_fast_out = fast score of the arrangement that is current after applying the pick. */
int hicmi_p2_decide_window(hicmi_ctx *ctx, int64_t first, int64_t k, double total, double floor, double cur_fast,
                           int64_t *pick_out, double *best_out, double *pick_fast_out);
/* The short lists behind bruteForceBestScore / scanOrdering's window steps (OG:457-466, 519-538), taken on the device
 * without downloading the deltas: for the `count` consecutive windows first, first+1, ... of k <= 8 scaffolds against
 * the current arrangement and tables (like hicmi_p2_score_window), the candidates c whose fast score
 *     fast[c] = delta[c] / total                                    (k == S)
 *     fast[c] = cur_fast + (delta[c] - delta[c0]) / total           (otherwise; c0 = identity order, current signs;
 *                                                                     cur_fast NaN: computed here)
 * is finite and >= top - |top| * 1e-9, top = max(floor, largest finite fast), in ascending candidate order, with their
 * fast scores: equal bit for bit to that rule applied to hicmi_p2_score_window's deltas.  Window w's list is
 * idx_out[w * cap ...] / fast_out[w * cap ...] with n_near_out[w] entries; n_near_out[w] > cap reports an overflow (that
 * window's list is not returned).  Windows of at least HICMI_P2_DEVICE_DECIDE scaffolds (default 7, "off": none) are
 * decided through these lists in hicmi_p2_decide_window and the scan calls. */
int hicmi_p2_window_shortlist(hicmi_ctx *ctx, int64_t first, int64_t count, int64_t k, double total, double floor,
                              double cur_fast, int64_t cap, int64_t *n_near_out, int64_t *idx_out, double *fast_out);
/* checkAllScores (OG:332-372) for scaffold new_id against the arrangement (ids, rev): computes the
 * literal total of "arrangement + new scaffold last" (OG:484-487, 343), scores the 2(S+1) candidates in
 * the reference's enumeration order (orientation tested first alternates with the gap, starting from
 * new_rev_now) and returns the winning gap / orientation (gap_out = -1: nothing scored above 0). */
int hicmi_p2_decide_insertion(hicmi_ctx *ctx, const int32_t *ids, const uint8_t *rev, int64_t S, int32_t new_id,
                              int32_t new_rev_now, int64_t *gap_out, int32_t *rev_out, double *best_out);

/* Whole loops, so that one chromosome costs a handful of host calls (chromosomes are independent and
 * are driven concurrently from host threads, one context each).
 * hicmi_p2_insert_all = orderRemainderScaffolds (OG:475-493): ids/rev hold the S0 ordered scaffolds on
 * entry and S0 + n_new on return (caller provides the capacity); new_ids are the remaining scaffolds
 * in pull order, each entering in '+' orientation.  best_out = bestCost of the last insertion.
 * hicmi_p2_scan_pass = one round of scanOrdering (OG:513-541) over windows of k scaffolds, every
 * winner applied before the next window; ids/rev updated in place, *best_io / *cur_fast_io carried,
 * *improved_out = 1 if any window improved (the reference's `stop`).
 * hicmi_p2_scan_all = the whole `while True` loop of scanOrdering (OG:509-547): rounds until one brings no
 * improvement, *rounds_out = how many ran ("Working on round i of final step..." is printed once per round by the caller). */
int hicmi_p2_insert_all(hicmi_ctx *ctx, int32_t *ids, uint8_t *rev, int64_t S0, const int32_t *new_ids, int64_t n_new,
                        double *best_out);
int hicmi_p2_scan_pass(hicmi_ctx *ctx, int32_t *ids, uint8_t *rev, int64_t S, int64_t k, double total, double *best_io,
                       double *cur_fast_io, int32_t *improved_out);
int hicmi_p2_scan_all(hicmi_ctx *ctx, int32_t *ids, uint8_t *rev, int64_t S, int64_t k, double total, double *best_io,
                      double *cur_fast_io, int64_t *rounds_out);
/* hicmi_p2_insert_all for n_jobs chromosomes at once (the loop over chromosomes of OG:608-612 turned
 * inside out): job j uses context ctxs[j] - its own selection and layout, all contexts on one device - and
 * the arrays ids[j] / rev[j] / new_ids[j] with S0[j] / n_new[j] entries as above.  The chromosomes advance
 * in lock step, every step of all of them decided on the device; best_out[j] as for hicmi_p2_insert_all.
 * Must not run concurrently with other calls on any of the contexts. */
int hicmi_p2_insert_all_multi(int64_t n_jobs, hicmi_ctx *const *ctxs, int32_t *const *ids, uint8_t *const *rev,
                              const int64_t *S0, const int32_t *const *new_ids, const int64_t *n_new, double *best_out);

/* The start of n_jobs chromosomes (OG:551-576 up to and including the brute force) in one call, one context each, all on
 * one device: for job j what hicmi_p2_select, hicmi_p2_layout, hicmi_p2_set_arrangement, hicmi_p2_arrangement_total,
 * hicmi_p2_window_tables and hicmi_p2_decide_window(0, k, total, 0., NaN) do, with the same results bit for bit and the
 * same state left in the context, but phase by phase over all jobs: a phase is queued on every job's stream before any
 * of them is waited for.
 * Flat inputs, job after job: sel (n_sel[j] matrix rows: the bins scaffold by scaffold, ascending), scaf_start / scaf_len
 * (n_scaf[j] ranges of that selection), first_ids (the k[j] scaffolds the brute force orders, all '+'; 1 <= k[j] <= 8,
 * k[j] <= n_scaf[j]).  orders[k] / orients[k] with n_orders[k] / n_orients[k] rows, k = 0 .. 8: the tables of
 * hicmi_p2_window_tables for every k that occurs (unused entries may be NULL).
 * Outputs per job: total_out (OG:448), status_out = 0 decided: pick_out = winning candidate (order index * n_orients +
 * orientation index), cost_out its literal cost; 1: total is 0 ("Zero contact values found", nothing was scored);
 * 2: no candidate scored above 0 (pick_out = -1).  Must not run concurrently with other calls on the contexts. */
int hicmi_p2_start_all(int64_t n_jobs, hicmi_ctx *const *ctxs, const int32_t *sel, const int64_t *n_sel,
                       const int32_t *scaf_start, const int32_t *scaf_len, const int64_t *n_scaf, const int32_t *first_ids,
                       const int64_t *k, const int8_t *const *orders, const int64_t *n_orders, const uint8_t *const *orients,
                       const int64_t *n_orients, double *total_out, int64_t *pick_out, double *cost_out, int32_t *status_out);
/* scanOrdering (OG:495-549) entered with the arrangement as the insertion calls return it: sets it, takes its total in
 * exactly that order (OG:506; *total_out), loads the window tables for k unless they are the loaded ones, then runs
 * hicmi_p2_scan_all from *best_io.  ids / rev updated in place. */
int hicmi_p2_scan_arranged(hicmi_ctx *ctx, int32_t *ids, uint8_t *rev, int64_t S, int64_t k, const int8_t *orders,
                           int64_t n_orders, const uint8_t *orients, int64_t n_orients, double *total_out, double *best_io,
                           int64_t *rounds_out);

/* Placement support of a finished ordering.  For one chromosome: its selection and layout (hicmi_p2_select,
 * hicmi_p2_layout), its final arrangement A = (ids, rev) of S scaffolds and ONE total (the caller's: the literal total
 * of the layout in layout order, every scaffold '+', so that all scores of a chromosome are on one footing).
 * scores_out[(j * S + g) * 2 + r] = objective, under that total, of "A without scaffold j, j put back at gap g
 * (0 ... S-1 of the arrangement without j) in orientation r (0 '+', 1 '-')": S x S x 2 doubles in enumeration order
 * (j, then g ascending, then '+' before '-'), closed form BASE - STRADDLE(g) + CROSS(g, r), fp64.  (g = j, r = rev[j])
 * is A itself; for a one-bin scaffold (g = j, the other r) has A's bin order too.
 * best_out[2 j] = 2 g + r of the first maximum, in enumeration order, of the closed-form scores over the candidates of
 * j whose bin order differs from A's - of a one-bin scaffold only its '+' candidates count, '-' being the same bin
 * order - or -1 when there is none (S = 1: the only other candidate is the whole chromosome read backwards, which is
 * not counted); best_out[2 j + 1] = how many of those candidates lie within 1e-9 (relative)
 * of that maximum.  1: the move is decided.  More: the caller re-scores them literally (hicmi_p2_score_exact) and the
 * first strict maximum of those values wins.
 * A chromosome of fewer than 2 bins, or with total <= 0, gets 0.0 everywhere and no candidate.
 * More than 4096 scaffolds or 40960 bins in one chromosome: HICMI_EUNSUPPORTED.
 * hicmi_p2_support_multi: n_jobs chromosomes (one context each, all on one device) in one pair of launches - the grid
 * runs over (chromosome, left-out scaffold) records - and one download.  Matrix reads are O(S n^2) per chromosome.
 * Replaces the contexts' current arrangement by A.  Must not run concurrently with other calls on the contexts. */
int hicmi_p2_support(hicmi_ctx *ctx, const int32_t *ids, const uint8_t *rev, int64_t S, double total, double *scores_out,
                     int32_t *best_out);
int hicmi_p2_support_multi(int64_t n_jobs, hicmi_ctx *const *ctxs, const int32_t *const *ids, const uint8_t *const *rev,
                           const int64_t *S, const double *totals, double *const *scores_out, int32_t *const *best_out);

/* Break support of a finished ordering: every scaffold cut at every bin boundary.  Chromosome, arrangement A = (ids,
 * rev) of S scaffolds and the ONE total are as for hicmi_p2_support.  Scaffold j occupies L positions of A, read as
 * laid down (a '-' scaffold reads descending); cut p = 1 ... L-1 makes the left piece P, the first p positions, and
 * the right piece Q, the rest.  Candidate k = 4 w + 2 x + y of (j, p): pieces swapped (w), P reversed (x), Q reversed
 * (y), every other position of A unchanged; k = 0 is A and k = 7 the whole scaffold flipped in place.
 * scores_out: for the scaffolds in arrangement order, scaffold j's (L_j - 1) x 8 block [8 (p - 1) + k] = objective of
 * that candidate under `total`, closed form, fp64; the blocks are concatenated (a one-bin scaffold has none), sum of
 * 8 (L_j - 1) doubles in all, and the caller computes the offsets.
 * A candidate competes if both pieces have at least min_piece (>= 1) bins and its bin order differs from A's, from the
 * in-place whole flip's and from every earlier candidate's of the same cut: x = 1 never with |P| = 1, y = 1 never with
 * |Q| = 1; of the rest k = 0 and 7 are out, k = 5 when |P| = 1, k = 6 when |Q| = 1, k = 4 when both pieces have one bin.
 * best_out[2 j] = 8 (p - 1) + k of the first maximum, in enumeration order (p ascending, then k), of the closed-form
 * scores over j's competing candidates, or -1 when none competes (L = 1, L = 2, min_piece); best_out[2 j + 1] = how
 * many of them lie within 1e-9 (relative) of that maximum.  1: decided.  More: the caller re-scores them literally
 * (hicmi_p2_score_exact) and the first strict maximum of those values wins.
 * A chromosome of fewer than 2 bins, or with total <= 0, gets 0.0 everywhere and no candidate.
 * More than 40960 bins in one chromosome, or more than 2^31 - 1 workgroups in one call (a scaffold of L bins takes
 * about L^2 / 4): HICMI_EUNSUPPORTED.
 * hicmi_p2_breaks_multi: n_jobs chromosomes (one context each, all on one device) in one pair of launches - the grid
 * runs over (chromosome, scaffold of at least 2 bins) records - and one download.  Replaces the contexts' current
 * arrangement by A.  Must not run concurrently with other calls on the contexts. */
int hicmi_p2_breaks(hicmi_ctx *ctx, const int32_t *ids, const uint8_t *rev, int64_t S, double total, int64_t min_piece,
                    double *scores_out, int32_t *best_out);
int hicmi_p2_breaks_multi(int64_t n_jobs, hicmi_ctx *const *ctxs, const int32_t *const *ids, const uint8_t *const *rev,
                          const int64_t *S, const double *totals, int64_t min_piece, double *const *scores_out,
                          int32_t *const *best_out);

/* Inversion support of a finished ordering: every run of consecutive scaffolds read backwards.  Chromosome, arrangement
 * A = (ids, rev) of S scaffolds, arr_pos[k] = first position of scaffold k in A and the ONE total are as for
 * hicmi_p2_support.  Candidate (i, j), 0 <= i <= j < S, is A with its positions [a, b) = [arr_pos[i], arr_pos[j + 1])
 * read backwards: scaffolds i ... j in reverse order, each flipped, every other position unchanged.  Pairs inside the
 * segment and pairs outside it keep their distance, so with c = a + b - 1 and h(d) = H[n - 1] - H[d - 1]
 *     total * (score(i, j) - score0) = sum_{t in [a, b)} [ sum_{o < a}  M[t][o] (h(c - t - o) - h(t - o))
 *                                                         + sum_{o >= b} M[t][o] (h(o + t - c) - h(o - t)) ],
 * t and o positions of A and M read through A's bin order.
 * scores_out[i * S + j] = objective of candidate (i, j) under `total`, closed form, fp64: S x S doubles.  j < i holds
 * 0.0; j = i is scaffold i flipped in place (hicmi_p2_support's scores_out[(i * S + i) * 2 + 1 - rev[i]]); j > i is the
 * segment reversal.  max_span > 0: segments of more than max_span scaffolds are not computed and hold 0.0.
 * A candidate competes if j > i, it is not (0, S - 1) - the chromosome read backwards, the same objective - and, when
 * max_span > 0, j - i + 1 <= max_span.  best_out[2 i] = j of the first maximum, j ascending, of the closed-form scores
 * over the competing candidates with left end i, or -1 when none competes (the last scaffold; S = 2);
 * best_out[2 i + 1] = how many of them lie within 1e-9 (relative) of that maximum.  1: decided.  More: the caller
 * re-scores them literally (hicmi_p2_score_exact) and the first strict maximum of those values wins.
 * A chromosome of fewer than 2 bins, or with total <= 0, gets 0.0 everywhere and no candidate.
 * The call reads sum of len * (n - len) matrix elements over its computed candidates, len = b - a; the host adds that
 * up first and a call above 1e13 returns HICMI_EUNSUPPORTED naming max_span, as does one of more than 4096 scaffolds or
 * 40960 bins in a chromosome or 2^31 - 1 workgroups (one per computed candidate).  Scratch: 64 doubles per chromosome.
 * hicmi_p2_inversions_multi: n_jobs chromosomes (one context each, all on one device) in one pair of launches - the
 * grid runs over (chromosome, left end) records - and one download.  The sums are added in a fixed order: two calls
 * give the same bits.  Replaces the contexts' current arrangement by A.  Must not run concurrently with other calls
 * on the contexts. */
int hicmi_p2_inversions(hicmi_ctx *ctx, const int32_t *ids, const uint8_t *rev, int64_t S, double total, int64_t max_span,
                        double *scores_out, int32_t *best_out);
int hicmi_p2_inversions_multi(int64_t n_jobs, hicmi_ctx *const *ctxs, const int32_t *const *ids, const uint8_t *const *rev,
                              const int64_t *S, const double *totals, int64_t max_span, double *const *scores_out,
                              int32_t *const *best_out);

/* ---- Part 3 input scan (host code, no GPU) -----------------------------------------------------
 * readValidPairFile (orientSmallScaffolds.py:159-177): of a HiC-Pro allValidPairs file
 * (read, scaffold1, pos1, strand1, scaffold2, pos2, ...) keep the lines whose (scaffold1, scaffold2) is one of the
 * registered ORDERED name pairs.  names_blob / name_off[n_names + 1]: the scaffold names, concatenated;
 * pair_a / pair_b: name indices of the n_pairs registered pairs.  hicmi_scan_valid_pairs parses the file with
 * `threads` host threads (0 = all) and returns the number of hits and of lines; hicmi_scan_fetch copies the hits
 * out in file order - (registered pair, pos1, pos2) - and releases the handle.  A line with fewer than six
 * columns or a non-integer position of a registered pair is an error, as in the reference. */
int hicmi_scan_valid_pairs(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                           const int32_t *pair_a, const int32_t *pair_b, int64_t n_pairs, int threads,
                           int64_t *n_hits_out, int64_t *n_lines_out, void **handle_out);
int hicmi_scan_fetch(void *handle, int32_t *pair_idx, int64_t *pos1, int64_t *pos2);

/* ---- raw contact maps from the valid pairs: HiC-Pro's build_matrix at any bin size -----------------
 * Scaffold s of the size file (names_blob / name_off / scaf_size, in the file's order) has ceil(size / resolution)
 * bins from its own start; end (s, pos), pos 1-based, falls in bin first_bin[s] + (pos - 1) / resolution.  A pair with
 * both ends in one bin adds 1 to C[i][i], any other pair 1 to C[i][j] and 1 to C[j][i]: the dense convention of
 * hicmi_load_hicpro_matrix and hicmi_rebin, so the upper triangle with the diagonal sums to the pairs used.
 *
 * hicmi_parse_valid_pairs (host code, no GPU): the chunked form of hicmi_scan_valid_pairs that keeps every line.  It
 * parses whole lines from first_byte (a line start; 0 at first) until max_pairs pairs are kept or the file ends, with
 * `threads` host threads (0 = all); next_byte_out is where the next call starts and equals the file size when the file is
 * done.  A call that reaches max_pairs stops right after the line of its last pair, so the kept pairs - in file order -
 * the statistics and next_byte_out depend on the file and max_pairs alone, not on `threads`.  The four output arrays
 * hold max_pairs entries.  stats4: lines read, pairs kept, lines naming a scaffold that is not in the name list
 * (skipped), lines with a position below 1 or above the scaffold's size (skipped).  CRLF line ends, a last line without
 * a newline, an empty file and lines of more than six columns are accepted.  HICMI_EINVAL with "malformed valid-pair
 * line at byte <offset>": fewer than six columns (an empty line too) or a position that is not an integer.
 *
 * hicmi_map_begin / hicmi_map_add_pairs / hicmi_map_finish: one map, counted on the device from host arrays of pairs
 * (scaffold indices and 1-based positions).  begin allocates m x m zeroed unsigned 64-bit counts as scratch - the
 * context's matrix state is untouched until finish - and gives up a build that was open.  add_pairs checks every index
 * and position on the host first (HICMI_EINVAL, nothing uploaded, the open build unchanged), uploads the arrays and
 * counts the cell (min(i, j), max(i, j)) of every pair with one 64-bit integer atomic add per pair;
 * HICMI_BUILDMAP_PLAIN=0 in the environment takes the combining kernel instead (the A/B: a workgroup brings the equal
 * cells of its slice of pairs together in a hash table in LDS and issues one atomic add per distinct cell, carrying its
 * multiplicity; =1 names the default).  Integer adds: both forms, any split into calls and any arrival order give the
 * same bits.  finish converts the counts to doubles (exact below 2^53), mirrors the strict
 * upper triangle into the lower one and installs the result like hicmi_rebin: owned by the context, ld = m, both row
 * sums recomputed; pairs_out (may be NULL): the pairs added.  HICMI_EINVAL: add_pairs or finish without begin, a
 * resolution below 1, a negative size, no bins; HICMI_EUNSUPPORTED: more than 65,536 bins.  After any error the
 * context's matrix state is as before, and hicmi_destroy releases an open build.
 *
 * hicmi_build_maps: one pass over the pair file for n_res maps, ctxs[k] at resolution[k], all contexts distinct and on
 * one device.  Chunks of pairs (2^22 by default, HICMI_BUILDMAP_CHUNK_PAIRS=<n> in the environment) come from
 * hicmi_parse_valid_pairs into pinned memory, each is uploaded once and counted into every map, and the next chunk is
 * parsed meanwhile.  stats5: the four of stats4 over the whole file, then the number of chunks.  Every resolution is
 * checked before the file is read; on any error no context's matrix state has changed. */
int hicmi_parse_valid_pairs(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                            const int64_t *scaf_size, int threads, int64_t first_byte, int64_t max_pairs,
                            int32_t *scaf_a, int64_t *pos_a, int32_t *scaf_b, int64_t *pos_b,
                            int64_t *n_out, int64_t *next_byte_out, int64_t *stats4);
int hicmi_map_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, int64_t resolution);
int hicmi_map_add_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a,
                        const int32_t *scaf_b, const int64_t *pos_b, int64_t n);
int hicmi_map_finish(hicmi_ctx *ctx, int64_t *pairs_out);
int hicmi_build_maps(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                     const int64_t *scaf_size, int64_t n_res, const int64_t *resolution, hicmi_ctx *const *ctxs,
                     int threads, int64_t *stats5);

/* ---- contact maps of the assembled genome: the pairs counted in chromosome coordinates ------------------
 * An assembly lays scaffolds end to end into n_seq sequences of the sizes seq_size.  Per scaffold of the size file:
 * lift_seq (the sequence it lies in, -1: dropped), lift_off (its offset there, >= 0) and lift_rev (non-zero: reversed).
 * The 1-based position p on a scaffold of length L becomes off + p, or off + L - p + 1 on a reversed scaffold, on its
 * sequence; bins and counts are those of 9l applied to the sequences: ceil(seq_size / resolution) bins per sequence, cut
 * from its own start.  A pair with an end on a dropped scaffold is skipped and counted as unlifted.
 *
 * hicmi_map_begin_lifted is hicmi_map_begin for such a build: m and first_bin come from seq_size, the tables stay on the
 * device with the build.  hicmi_map_add_pairs (which still checks indices and positions against the scaffold sizes) and
 * hicmi_map_finish (whose pairs_out leaves the unlifted pairs out) then work as in 9l.  HICMI_LIFTMAP_PLAIN=1|0 in the
 * environment names the counting kernel of a lifted build as HICMI_BUILDMAP_PLAIN does for a plain one; it is read at
 * every call.  HICMI_EINVAL, before anything is allocated, with a message naming the scaffold: lift_seq outside
 * -1 .. n_seq - 1, a negative offset or size, lift_off + size beyond seq_size[lift_seq], two scaffolds of non-zero size
 * that overlap in one sequence; HICMI_EUNSUPPORTED: more than 65,536 bins.  After an error the matrix state and an open
 * build are as the 9l calls leave them.
 *
 * hicmi_pair_stats: the statistics of a chunk of pairs (host arrays) under the lift, computed on the context's device
 * and ADDED to the outputs; it has no matrix state and touches none.  Over the lifted pairs: a pair is cis when both
 * ends lie in one sequence, else trans; seq_cis_out[s] counts the cis pairs of s, seq_trans_out[s] the trans pairs with
 * an end in s (a trans pair counts in two sequences); decay_out[256] is the histogram of d = |p'_a - p'_b| over cis
 * pairs - slot 0 holds d = 0, d >= 1 falls in slot 1 + 4 e + (((d - 2^e) * 4) >> e), e = floor(log2 d) (quarter
 * octaves; slots above 252 stay 0); *unlifted_out counts the skipped pairs.  All unsigned 64-bit integers: every
 * chunking and arrival order gives the same bits.
 *
 * hicmi_lift_maps is hicmi_build_maps with the lift tables and the statistics outputs: one pass over the file, n_res
 * lifted maps and the statistics of every chunk, added to the outputs when the whole file is counted.  stats5 as in
 * hicmi_build_maps.  On an error before every chunk is counted - a resolution or a table refused, the file, a malformed
 * line, a HIP error while counting - no context's matrix state and no output changes.  The maps are installed one
 * context after the other only then; should an installation itself fail (the row-sum buffers cannot be allocated, a HIP
 * error in the conversion), the contexts before it hold their new maps, that one is as the failed step left it, those
 * after it keep what they held, and the outputs are unchanged.  hicmi_build_maps installs in the same way. */
int hicmi_map_begin_lifted(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                           const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                           int64_t resolution);
int hicmi_pair_stats(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b,
                     const int64_t *pos_b, int64_t n, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                     const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                     uint64_t *decay_out, uint64_t *seq_cis_out, uint64_t *seq_trans_out, uint64_t *unlifted_out);
int hicmi_lift_maps(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                    const int64_t *scaf_size, const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev,
                    const int64_t *seq_size, int64_t n_seq, int64_t n_res, const int64_t *resolution,
                    hicmi_ctx *const *ctxs, int threads, int64_t *stats5, uint64_t *decay_out, uint64_t *seq_cis_out,
                    uint64_t *seq_trans_out, uint64_t *unlifted_out);

/* ---- spanning depth: the read pairs with one end on each side of every cut and junction --------------
 * The assembly is given by the lift tables of 9m, checked in the same way.  Every placed scaffold of size L > 0 is cut
 * into ceil(L / step) cells from its left end as it lies in its sequence: position p falls in local cell (p - 1) / step,
 * on a reversed scaffold in (L - p) / step.  The cells are numbered in one order, sequences ascending and inside a
 * sequence by offset; gaps hold none.  cell_first_out[s] is the first cell of scaffold s, -1 for a dropped or empty one.
 * Slot c stands for the boundary after cell c; the last cell of a sequence is its terminator.  A pair whose ends lift to
 * one sequence, at most max_span apart when max_span is not 0, with the cells ca < cb adds +1 at slot ca and -1 at slot
 * cb; D, the inclusive prefix sum of the marks, is the number of counted pairs with cell(a) <= c < cell(b), and 0 at every
 * terminator.  counters5: pairs that marked, cis pairs within max_span in one cell, cis pairs beyond max_span, trans
 * pairs, unlifted pairs.  Unsigned 64-bit integers throughout: every chunking and arrival order gives the same bits.
 *
 * hicmi_span_begin checks the tables, returns the numbering and allocates zeroed marks; a span build that was open is
 * given up.  The context's matrix state and an open map build (9l, 9m) are never touched by these calls.
 * hicmi_span_add_pairs checks every index and position on the host like hicmi_map_add_pairs (HICMI_EINVAL, nothing
 * uploaded, the build unchanged), uploads the arrays and marks them.  HICMI_SPANS_PLAIN=1 in the environment, read at
 * every call, takes two global atomic adds per marking pair; =0 and the default take the combining kernel, in which a
 * workgroup sums the marks of its slice per slot in a table in LDS first.  Both give the same bits.
 * hicmi_span_finish scans the marks into D and D into S and answers the n_rec records (lo, hi, q0, q1) of 4 integers each:
 * [q0, q1) must be the cells of one sequence and q0 <= lo <= hi < q1.  With Lsum(c) = D[c-F] + .. + D[c-1] and
 * Rsum(c) = D[c+1] + .. + D[c+F], F = flank, slot c competes when c - F >= q0, c + F <= q1 - 2 and min(Lsum, Rsum) > 0;
 * its ratio is (double)(D[c] F) / (double)min(Lsum, Rsum).  picks_out[4 r ..] = slot, D, Lsum, Rsum of the competing slot
 * of [lo, hi] with the lowest ratio, the lowest slot among equal ratios; slot -1 (and zeros) when none competes.
 * depth_out (may be NULL) receives D of every cell.  The build is closed.  HICMI_EINVAL, the build left open and
 * unchanged: no open build, a flank outside 1 .. 4096, a record that is not a slot range inside one sequence.
 * HICMI_EINVAL at begin: step < 1, max_span < 0, tables refused, no cells; HICMI_EUNSUPPORTED: more than 2^27 cells, or
 * (at finish, which closes the build) pairs x flank could reach 2^53.
 *
 * hicmi_span_file: begin, every pair of the file, finish, in one pass with the chunked parser as in hicmi_build_maps
 * (HICMI_BUILDMAP_CHUNK_PAIRS, stats5 as there).  Tables, flank and records are refused before the file is read; on any
 * error no output is written, and no span build stays open. */
int hicmi_span_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                     const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                     int64_t step, int64_t max_span, int64_t *cell_first_out, int64_t *n_cells_out);
int hicmi_span_add_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a,
                         const int32_t *scaf_b, const int64_t *pos_b, int64_t n);
int hicmi_span_finish(hicmi_ctx *ctx, int64_t flank, const int64_t *recs, int64_t n_rec, int64_t *picks_out,
                      uint64_t *counters5_out, uint64_t *depth_out);
int hicmi_span_file(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                    const int64_t *scaf_size, const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev,
                    const int64_t *seq_size, int64_t n_seq, int64_t step, int64_t max_span, int64_t flank,
                    const int64_t *recs, int64_t n_rec, hicmi_ctx *ctx, int threads, int64_t *stats5, int64_t *picks_out,
                    uint64_t *counters5_out, uint64_t *depth_out, int64_t *cell_first_out, int64_t *n_cells_out);

/* ---- end support: the read pairs that link the ends of neighbouring scaffolds ------------------------
 * The assembly is given by the lift tables of 9m, checked in the same way.  The placed scaffolds of size > 0 are ranked
 * 0 .. P - 1 in the order 9n numbers cells: sequences ascending, inside a sequence by offset, then by index; rank_out[s]
 * is -1 for a dropped or empty scaffold, and gaps play no part.  A read end at position p of a scaffold of length L has
 * the lying coordinate x = L - p on a reversed scaffold, else p - 1.  With wl = min(window, L - L / 2) and
 * wr = min(window, L / 2) its zone is LEFT (0) when x < wl, RIGHT (1) when x >= L - wr, else MIDDLE.  A pair is, in this
 * order: unlifted (an end on a dropped scaffold), trans (two sequences), same (one scaffold), too far (the ranks differ
 * by d > reach), middle (either zone is MIDDLE), else linked.  table_out holds P x reach x 4 unsigned 64-bit counters: a
 * linked pair whose lower-rank scaffold has the rank i and the zone za there, and the zone zb at its other end, adds 1 at
 * ((i * reach + (d - 1)) * 4 + za * 2 + zb).  An entry whose i + d leaves the sequence of i stays 0.  counters6: linked,
 * middle, same, too far, trans, unlifted pairs.  Every chunking and arrival order gives the same bits.
 *
 * hicmi_ends_begin checks the tables, returns the ranks and P and allocates a zeroed table; an ends build that was open
 * is given up.  The context's matrix state, an open map build (9l, 9m) and an open span build (9n) are never touched by
 * these calls.  HICMI_EINVAL: window < 1, reach outside 1 .. 64, tables refused, no placed scaffold; HICMI_EUNSUPPORTED:
 * P x reach x 4 above 2^27; all before anything is allocated.
 * hicmi_ends_add_pairs checks every index and position on the host like hicmi_map_add_pairs (HICMI_EINVAL, nothing
 * uploaded, the build unchanged), uploads the arrays and counts them.  HICMI_ENDS_PLAIN=1 in the environment, read at
 * every call, takes one global atomic add per linked pair; =0 and the default take the combining kernel, in which a
 * workgroup sums the pairs of its slice per counter in a table in LDS first.  Both give the same bits.
 * hicmi_ends_finish downloads the table and the counters and closes the build; HICMI_EINVAL without an open build.
 *
 * hicmi_ends_file: begin, every pair of the file, finish, in one pass with the chunked parser as in hicmi_span_file
 * (HICMI_BUILDMAP_CHUNK_PAIRS, stats5 as there).  Tables, window and reach are refused before the file is read; on any
 * error no output is written, and no ends build stays open. */
int hicmi_ends_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                     const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                     int64_t window, int64_t reach, int32_t *rank_out, int64_t *n_placed_out);
int hicmi_ends_add_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a,
                         const int32_t *scaf_b, const int64_t *pos_b, int64_t n);
int hicmi_ends_finish(hicmi_ctx *ctx, uint64_t *table_out, uint64_t *counters6_out);
int hicmi_ends_file(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                    const int64_t *scaf_size, const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev,
                    const int64_t *seq_size, int64_t n_seq, int64_t window, int64_t reach, hicmi_ctx *ctx, int threads,
                    int64_t *stats5, uint64_t *table_out, uint64_t *counters6_out, int32_t *rank_out,
                    int64_t *n_placed_out);

/* ---- anchoring: the read pairs that link the scaffolds an ordering leaves out to the placed ones ------
 * The assembly is given by the lift tables of 9m, checked in the same way, and the placed scaffolds of size > 0 are
 * ranked as in 9p; seq_first[q] is the first rank of sequence q and S_q = seq_first[q + 1] - seq_first[q].  A candidate
 * is a dropped scaffold (lift_seq = -1) of size > 0; the candidates are taken in index order and each owns a block of
 * counters of one table, first_out[s] being the block's offset and -1 for a scaffold that is no candidate.
 *   target == NULL (sequence mode): every dropped scaffold of size > 0 is a candidate with a block of n_seq counters; a
 *     pair with one end on the candidate c and the other in sequence q adds 1 at first[c] + q.
 *   target != NULL (rank mode; int32 per scaffold): the candidates are the scaffolds with target[s] >= 0, the block of c
 *     has 4 x S_target[c] counters, and a pair whose placed end lies on the scaffold of rank r of sequence q = target[c]
 *     adds 1 at first[c] + (r - seq_first[q]) * 4 + zu * 2 + zp: zu is the half of c its own end p falls in, in the +
 *     coordinates of c (0 when p - 1 < L - L / 2, else 1), zp the zone of the placed end as it lies (9p; 0 left, 1 right).
 * counters6: anchored, middle (rank mode: the placed end in no zone), elsewhere (rank mode: the placed end in a sequence
 * other than the target), skipped (rank mode: the dropped end on a scaffold with target < 0), unplaced (neither end
 * lifts; two ends on one dropped scaffold too), placed (both ends lift); a pair is checked for placed, unplaced, skipped,
 * elsewhere and middle in this order.  Every chunking and arrival order gives the same bits.
 *
 * hicmi_anchor_begin checks the tables, returns the blocks and the size of the table and allocates a zeroed table; an
 * anchor build that was open is given up.  The context's matrix state, an open map build (9l, 9m), an open span build
 * (9n) and an open ends build (9p) are never touched by these calls.  HICMI_EINVAL, the message naming the scaffold:
 * tables refused, window < 1 (in either mode), no candidate, a target outside -1 .. n_seq - 1, a target >= 0 on a placed
 * or an empty scaffold, a target sequence with S_q = 0; HICMI_EUNSUPPORTED: more than 2^27 counters, or in rank mode more
 * than 2^25 placed scaffolds; all before anything is allocated.
 * hicmi_anchor_add_pairs checks every index and position on the host like hicmi_map_add_pairs (HICMI_EINVAL, nothing
 * uploaded, the build unchanged), uploads the arrays and counts them.  HICMI_ANCHOR_PLAIN=1 in the environment, read at
 * every call, takes one global atomic add per anchored pair; =0 and the default take the combining kernel, in which a
 * workgroup sums the pairs of its slice per counter in a table in LDS first.  Both give the same bits.
 * hicmi_anchor_finish downloads the table and the counters and closes the build; HICMI_EINVAL without an open build.
 *
 * hicmi_anchor_file: begin, every pair of the file, finish, in one pass with the chunked parser as in hicmi_span_file
 * and hicmi_ends_file (HICMI_BUILDMAP_CHUNK_PAIRS, stats5 as there).  Tables, targets and window are refused before the
 * file is read; on any error no output is written, and no anchor build stays open. */
int hicmi_anchor_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                       const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                       const int32_t *target, int64_t window, int64_t *first_out, int64_t *n_table_out);
int hicmi_anchor_add_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a,
                           const int32_t *scaf_b, const int64_t *pos_b, int64_t n);
int hicmi_anchor_finish(hicmi_ctx *ctx, uint64_t *table_out, uint64_t *counters6_out);
int hicmi_anchor_file(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                      const int64_t *scaf_size, const int32_t *lift_seq, const int64_t *lift_off, const uint8_t *lift_rev,
                      const int64_t *seq_size, int64_t n_seq, const int32_t *target, int64_t window, hicmi_ctx *ctx,
                      int threads, int64_t *stats5, uint64_t *table_out, uint64_t *counters6_out, int64_t *first_out,
                      int64_t *n_table_out);

/* ---- the resident pair store: read pairs kept on the device between calls ----------------------------
 * A pair is kept when scaf_a != scaf_b.  A pair with both ends on one scaffold s is intra: it is not stored and adds 1
 * to intra[s] (unsigned 64-bit, one per scaffold).  The store is four device arrays, scaf_a int32, pos_a int64, scaf_b
 * int32, pos_b int64, and holds the kept pairs in the order they were added: it is the boolean mask of the input.  No
 * ordering counts an intra pair in a table of 9p or 9q: it is same (9p) or placed (9q) when its scaffold is placed and
 * unlifted (9p) or unplaced (9q) when it is dropped, so the resident calls count the kept pairs and add the sums of
 * intra[] over the placed and over the dropped scaffolds to these counters.
 *
 * hicmi_pairs_begin opens an empty store of HICMI_PAIRS_FIRST_PAIRS pairs (default 2^22, read per begin, 1 .. 2^31) and
 * the zeroed intra array, all or nothing.  HICMI_EINVAL: the context already has a store, a negative size.  The
 * context's matrix state and open map, span, ends and anchor builds are never touched by the hicmi_pairs_* calls.
 * hicmi_pairs_add checks every index and position on the host like hicmi_map_add_pairs (HICMI_EINVAL, nothing uploaded,
 * the store as before the call), uploads the arrays and appends the kept pairs.  The capacity at least doubles when it
 * runs out, by device-to-device copy; an allocation that fails is HICMI_ENOMEM and, like a HIP error, gives the store
 * up.  HICMI_PAIRS_PLAIN=1 in the environment, read at every call, takes one thread per pair, one atomic bump of the
 * length per kept pair and one global atomic add per intra pair: the store is then the same multiset in another order.
 * =0 and the default take the stable compaction (per-wave ballot, per-workgroup counts, a scan over the workgroups),
 * which sums the intra pairs of a slice per scaffold in LDS first.  Everything computed from either store has the same
 * bits.
 * hicmi_pairs_file: begin and every pair of the file in one pass with the chunked parser as in hicmi_ends_file
 * (HICMI_BUILDMAP_CHUNK_PAIRS, stats5 as there).  On any error no store is left and no output is written.
 * hicmi_pairs_info: the pairs kept, the intra pairs in all and, unless intra_out is NULL, intra[n_scaf].
 * hicmi_pairs_fetch downloads the store into arrays of n_kept elements.  hicmi_pairs_drop releases the store; the
 * context releases it as well.  All three are HICMI_EINVAL without a store.
 *
 * hicmi_ends_resident and hicmi_anchor_resident: the numbering, the refusals, the table and the counters of
 * hicmi_ends_file and hicmi_anchor_file with the store in place of the file, for any lift tables, as often as wanted;
 * HICMI_ENDS_PLAIN and HICMI_ANCHOR_PLAIN are honoured.  The store is only read.  HICMI_EINVAL: no store, scaf_size or
 * n_scaf other than the store's, an open ends (anchor) build on the context, which is left as it was.  Outputs are
 * written only when everything is down. */
int hicmi_pairs_begin(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf);
int hicmi_pairs_add(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b,
                    const int64_t *pos_b, int64_t n);
int hicmi_pairs_file(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                     const int64_t *scaf_size, hicmi_ctx *ctx, int threads, int64_t *stats5);
int hicmi_pairs_info(hicmi_ctx *ctx, int64_t *n_kept_out, uint64_t *n_intra_out, uint64_t *intra_out);
int hicmi_pairs_fetch(hicmi_ctx *ctx, int32_t *scaf_a, int64_t *pos_a, int32_t *scaf_b, int64_t *pos_b);
int hicmi_pairs_drop(hicmi_ctx *ctx);
int hicmi_ends_resident(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                        const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                        int64_t window, int64_t reach, uint64_t *table_out, uint64_t *counters6_out,
                        int32_t *rank_out, int64_t *n_placed_out);
int hicmi_anchor_resident(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                          const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                          const int32_t *target, int64_t window, uint64_t *table_out, uint64_t *counters6_out,
                          int64_t *first_out, int64_t *n_table_out);

/* ---- seat support: every placed scaffold taken out and re-placed from the resident pair store --------
 * The leave-one-out relocation test of SALSA (Ghurye et al. 2017, BMC Genomics 18:527), 3D-DNA (Dudchenko et al. 2017,
 * Science 356:92) and YaHS (Zhou et al. 2023, Bioinformatics 39:btac808) on the read pairs themselves.  The seat of a
 * scaffold is its chromosome, gap and orientation.  rank and seq_first are those of hicmi_ends_begin at reach 1.  A
 * placed scaffold c with a base, in sequence q with S_q such scaffolds, owns a block of n_seq + 4 S_q unsigned 64-bit
 * counters; the blocks lie in scaffold-index order and first_out[c] is the start of c's block, -1 for a dropped or empty
 * scaffold.  first[c] + q' counts the kept pairs between c and any other placed scaffold of sequence q'.
 * first[c] + n_seq + k * 4 + half * 2 + zone counts the pairs between a half of c (0: the first len - len / 2 bases in
 * c's own + coordinates) and an end zone (0 left, 1 right, as it lies, of `window` bases as in 9p) of the scaffold of
 * local rank k in c's own sequence; the row k = rank[c] - seq_first[q] exists and stays zero.  With that row deleted the
 * two parts of c's block are what hicmi_anchor_resident counts in sequence mode and in rank mode with target[c] = q on
 * the lift tables with c alone dropped.  A pair between two placed scaffolds adds to the blocks of both.
 * counters5_out: seated (at least one gap counter), middle (one sequence, both far ends in the middle), trans (two
 * sequences), same (one scaffold), unlifted (an end on a dropped scaffold); the intra pairs the store does not keep are
 * added as same or unlifted from intra[].  Their sum is the number of pairs.
 * HICMI_SEATS_PLAIN=1 in the environment, read at every call, takes one thread per pair and up to four global atomic
 * adds; =0 takes the combining kernel (equal counters of a slice summed in LDS first).  Both give the same bits, as do
 * every store order and mate order.  HICMI_EINVAL: no store, scaf_size or n_scaf other than the store's, window < 1,
 * tables that hicmi_map_begin_lifted refuses, no placed scaffold with a base.  HICMI_EUNSUPPORTED: a table of more than
 * 2^27 counters.  The store is only read; the context's matrix state and open map, span, ends and anchor builds are
 * never touched.  table_out has room for n_table counters (the caller numbers the blocks the same way first).  Outputs
 * are written only when everything is down. */
int hicmi_seats_resident(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                         const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                         int64_t window, uint64_t *table_out, uint64_t *counters5_out, int64_t *first_out,
                         int64_t *n_table_out);

/* ---- the end-link graph of all scaffolds: which scaffold ends are linked to which, before any ordering --
 * The question every Hi-C scaffolder starts from (LACHESIS, Burton et al. 2013, Nat Biotechnol 31:1119; SALSA; 3D-DNA;
 * YaHS), answered from the resident pair store without an order file.  A scaffold is read in its own + coordinates: the
 * zone of a read end is that of 9p without a reversal (left: the first min(window, len - len / 2) bases, right: the last
 * min(window, len / 2), middle: the rest).  A kept pair lies on the scaffolds lo < hi; its combination is LL, LR, RL or RR
 * (first letter: the zone on lo) or OTHER when an end is in a middle zone, and its key lo << 33 | hi << 3 | combination
 * (0 .. 4).  The keys are counted in a find-or-insert table in device memory (open addressing, linear probing, a 64-bit
 * compare-and-swap against the empty mark ~0, bounded probing) whose capacity is the smallest power of two that is at
 * least 1,024 and at least 2 min(n_kept, 5 n_scaf (n_scaf - 1) / 2): it is never more than half full and never grows.
 * hicmi_links_resident counts the store, compacts the used slots, sorts them by key and merges them into one row per
 * scaffold pair with at least one pair; the rows stay on the context.  n_rows_out: their number.  counters2_out: linked
 * (one of the four end combinations) and middle (OTHER); their sum is the pairs kept.
 * hicmi_links_fetch copies the rows, sorted by (lo, hi): lo and hi of n_rows entries, counts5 of n_rows x 5 row-major in
 * the order LL, LR, RL, RR, OTHER.  hicmi_pairs_drop releases the rows with the store, and hicmi_pairs_add makes them
 * stale: a fetch then needs a new count.  hicmi_links_info: of the last count the used slots (records), the slots of
 * its table and the milliseconds the host took to sort the records, for the measurements of 9t.
 * HICMI_LINKS_PLAIN=1 in the environment, read at every call, takes one thread and one find-or-insert per pair; =0 takes
 * the combining kernel (equal keys of a slice summed in LDS first).  Both give the same rows, as do every store order and
 * mate order.  HICMI_EINVAL: no store, scaf_size or n_scaf other than the store's, window < 1, a fetch or an info before a count.
 * HICMI_EUNSUPPORTED: n_scaf above 2^30, a table of more than 2^31 slots (the message names the number).  A refusal
 * leaves every output and the rows of an earlier call as they were.  The store is only read; the context's matrix state
 * and open builds are never touched. */
int hicmi_links_resident(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, int64_t window, int64_t *n_rows_out,
                         uint64_t *counters2_out);
int hicmi_links_fetch(hicmi_ctx *ctx, int32_t *lo, int32_t *hi, uint64_t *counts5);
int hicmi_links_info(hicmi_ctx *ctx, int64_t *n_records_out, int64_t *n_slots_out, double *sort_ms_out);

/* ---- the end-link graph on lifted ends: links between the ends of sequences of several scaffolds ---------
 * What a scaffolder's second and later rounds count: the paths of one round are the units of the next.  The tables are
 * those of hicmi_map_begin_lifted: scaffold s lies in sequence lift_seq[s] (-1: dropped) at the offset lift_off[s],
 * reversed when lift_rev[s] is not 0; seq_size[n_seq] are the sizes of the sequences, gaps included.  Both ends of a kept
 * pair are lifted.  An end on a dropped scaffold makes the pair `unlifted`, two ends in one sequence make it `inside`.
 * Otherwise the zone of an end is that of 9t on its lifted position in its sequence read left to right (the bases of a
 * gap belong to a zone and hold no read), the pair lies on the sequences lo < hi, and its combination and key are those
 * of 9t with sequence indices in place of scaffold indices: `linked` for LL, LR, RL and RR, `middle` for OTHER.
 * hicmi_links_lifted counts the store in one pass into a table of the capacity of 9t for n_seq sequences, compacts, sorts
 * and merges as hicmi_links_resident does; the rows replace those of an earlier hicmi_links_resident or
 * hicmi_links_lifted call on the context (and the other way round) and are read with hicmi_links_fetch, lo and hi being
 * sequence indices; hicmi_links_info reports on the call.  n_rows_out: their number.  counters4_out: linked, middle,
 * inside, unlifted; their sum is the pairs kept (the intra pairs of the store are not added).  With every scaffold its
 * own + sequence in index order the rows and the first two counters are those of hicmi_links_resident.
 * HICMI_LINKS_PLAIN is read at every call as in 9t; both forms give the same rows.  HICMI_EINVAL: no store, scaf_size or
 * n_scaf other than the store's, window < 1, a null pointer, tables that hicmi_map_begin_lifted refuses (n_seq < 1
 * among them).  HICMI_EUNSUPPORTED: n_seq above 2^30, a table of more than 2^31 slots.  n_seq = 1 and every scaffold
 * dropped are valid calls with zero rows.  A refusal leaves every output and the rows of an earlier call as they were.
 * The store is only read; the context's matrix state and open builds are never touched. */
int hicmi_links_lifted(hicmi_ctx *ctx, const int64_t *scaf_size, int64_t n_scaf, const int32_t *lift_seq,
                       const int64_t *lift_off, const uint8_t *lift_rev, const int64_t *seq_size, int64_t n_seq,
                       int64_t window, int64_t *n_rows_out, uint64_t *counters4_out);

/* ---- scaffolds cut into pieces: every read end moved from its scaffold to its piece -------------------
 * Scaffold s of the n_scaf scaffolds has the pieces piece_first[s] .. piece_first[s + 1] - 1 (int32, n_scaf + 1 entries,
 * ascending from 0 to n_piece), left to right; piece k starts after piece_start[k] bases of its parent (int64, 0 for a
 * first piece, strictly ascending inside a scaffold and below its size; a scaffold without a base has one piece).  The
 * end (s, p), 1 <= p <= scaf_size[s], goes to the last piece k of s with piece_start[k] < p, at p - piece_start[k].
 * The counters are 4 n_piece unsigned 64-bit integers, [within][sibling][other][mark] of n_piece each, and every call
 * ADDS to them: a pair with both ends in piece k adds 1 to within[k]; a pair in two pieces of one scaffold adds 1 to
 * sibling of both, 1 to mark of the lower and -1 (mod 2^64) to mark of the higher piece; a pair in pieces of two scaffolds
 * adds 1 to other of both.  The prefix sum of mark over the pieces of a scaffold is, at piece k, the number of pairs with
 * one end at or before the last base of k and one after it.  Every chunking and arrival order gives the same bits.
 * HICMI_EINVAL for tables that are not so (the message names the scaffold), before anything else is looked at.
 *
 * hicmi_split_pairs works on host arrays: every index and position is checked on the host like hicmi_map_add_pairs
 * (HICMI_EINVAL, nothing uploaded, no output written), then the chunk is moved on the device.  It touches no matrix
 * state, no open map build and no open span build.  HICMI_SPLIT_PLAIN=1 in the environment, read at every call, takes
 * the definition literally - a scan over the pieces of the scaffold and one global atomic add per counter and pair; =0
 * and the default take an uncut scaffold as its one piece, bisect a cut one, and sum the contributions of a workgroup
 * per counter in a table in LDS first.  Both give the same bits.
 *
 * hicmi_split_maps is hicmi_build_maps on the pieces: one pass over the file with the chunked parser, which reads the
 * scaffolds' names and sizes; each chunk is uploaded once, moved once and counted into the map of every resolution, cut
 * from the pieces (HICMI_BUILDMAP_CHUNK_PAIRS, HICMI_BUILDMAP_PLAIN, stats5 and the all-or-nothing installation as
 * there).  n_res = 0 computes the counters alone; ctxs[0] must then still be a context, which lends its device and its
 * stream and is left as it is.  Tables and resolutions are refused before the file is read; on any error no context and
 * no counter changes.
 *
 * hicmi_split_valid_pairs (host code, no GPU) writes path_out: every line of path_in that hicmi_parse_valid_pairs keeps,
 * with its columns 1, 2 and 4, 5 replaced by the name of the piece (piece_names_blob, piece_name_off as names_blob,
 * name_off) and the position in the piece, every other byte - further columns, CR LF, a missing last newline - as it
 * was; the lines the parser skips are dropped.  stats4 as hicmi_parse_valid_pairs fills it.  A malformed line is the
 * parser's error with its byte offset.  The file is written under another name and renamed when it is whole, so an
 * error leaves no output; the bytes do not depend on `threads`. */
int hicmi_split_pairs(hicmi_ctx *ctx, const int32_t *scaf_a, const int64_t *pos_a, const int32_t *scaf_b,
                      const int64_t *pos_b, int64_t n, const int64_t *scaf_size, int64_t n_scaf,
                      const int32_t *piece_first, const int64_t *piece_start, int64_t n_piece, int32_t *piece_a_out,
                      int64_t *pos_a_out, int32_t *piece_b_out, int64_t *pos_b_out, uint64_t *counters_out);
int hicmi_split_maps(const char *path, const char *names_blob, const int64_t *name_off, int64_t n_names,
                     const int64_t *scaf_size, const int32_t *piece_first, const int64_t *piece_start, int64_t n_piece,
                     int64_t n_res, const int64_t *resolution, hicmi_ctx *const *ctxs, int threads, int64_t *stats5,
                     uint64_t *counters_out);
int hicmi_split_valid_pairs(const char *path_in, const char *path_out, const char *names_blob, const int64_t *name_off,
                            int64_t n_names, const int64_t *scaf_size, const int32_t *piece_first,
                            const int64_t *piece_start, int64_t n_piece, const char *piece_names_blob,
                            const int64_t *piece_name_off, int threads, int64_t *stats4);

/* ---- plot support -----------------------------------------------------------------------------
 * plotContactMap (plotContactMaps.py:15-91) colours every cell of an N x N matrix between two
 * numpy.percentile limits.  The matrix stays on the device: kind 0 = raw contacts (Part 2 plots,
 * OG:619,704), 1 = distance transform (S2C:147 -> S2C:1124), 2 = similarity transform (S2C:149 ->
 * S2C:1156); order = the n_sel matrix rows shown, in plot order (NULL: all rows as stored).
 * hicmi_plot_percentiles: out[i] = numpy.percentile(cells, q[i]) (method "linear"), exact.
 * hicmi_plot_downsample: out = px x px block means (row-major fp64), px <= n_sel. */
int hicmi_plot_percentiles(hicmi_ctx *ctx, int kind, const int32_t *order, int64_t n_sel, const double *q, int64_t n_q,
                           double *out);
int hicmi_plot_downsample(hicmi_ctx *ctx, int kind, const int32_t *order, int64_t n_sel, int64_t px, double *out);

/* ---- Part 1: HMM boundary finder (hmm = True, S2C:730-942) -----------------------------------------
 * hmmChromosomes (S2C:754-819) fits hmmlearn's GaussianHMM(n_components=2, covariance_type="diag", n_iter=1000,
 * init_params="cm", params="cmt") to X = logTransformMatrix(similarity)[c:n, c:p] (S2C:785-786, S2C:165-183) and
 * decodes it.  These entry points restate that model's numerics on the device; the host keeps
 * the control flow, the k-means++ draws and the convergence tests.  X lives in the context (T x D, row-major).
 *
 * hicmi_hmm_load_obs: X[t][d] = log10(sim + 1) (0 where sim == 0) of rows c + t and columns c + d of the similarity
 * matrix (S2C:149) in the row / column order `order` (n int32); T = n - c, D = p - c.  Needs hicmi_row_sums.
 * hicmi_hmm_set_obs / hicmi_hmm_get_obs: an arbitrary X in (tests), rows [row0, row0 + nrows) of the current view out.
 * hicmi_hmm_set_width: later rounds of one boundary use columns [0, D) of the X already built (S2C:786 with a smaller
 * prevCutInd), without a rebuild; every call below works on that view. */
int hicmi_hmm_load_obs(hicmi_ctx *ctx, const int32_t *order, int64_t n, int64_t c, int64_t p);
int hicmi_hmm_set_obs(hicmi_ctx *ctx, const double *X, int64_t T, int64_t D);
int hicmi_hmm_set_width(hicmi_ctx *ctx, int64_t D);
int hicmi_hmm_get_obs(hicmi_ctx *ctx, int64_t row0, int64_t nrows, double *out);
/* GaussianHMM._init (S2C:796-801): the k-means of the means (sklearn KMeans(n_clusters=2)) and the covariances
 * diag(numpy.cov(X.T)) + min_covar.
 * hicmi_hmm_dist2: out[j][t] = sum_d (X[t][d] - X[rows[j]][d])^2, k = 1 or 2 rows - the distances k-means++ seeding
 * draws from (the host draws the indices).
 * hicmi_hmm_col_stats: mean and sum of squared deviations from it of every column (var ddof=1 = m2 / (T - 1)).
 * hicmi_hmm_kmeans: Lloyd from centers_in (2 x D) as sklearn's _kmeans_single_lloyd runs it - stop when no label
 * changed, or when the summed squared center shift is <= tol, or after max_iter iterations; an empty cluster keeps
 * its center; labels ties go to cluster 0.  centers_out (2 x D), labels_out (T int32, may be NULL), inertia_out (may be
 * NULL), n_iter_out (may be NULL). */
int hicmi_hmm_dist2(hicmi_ctx *ctx, const int64_t *rows, int64_t k, double *out);
int hicmi_hmm_col_stats(hicmi_ctx *ctx, double *mean_out, double *m2_out);
int hicmi_hmm_kmeans(hicmi_ctx *ctx, const double *centers_in, int64_t max_iter, double tol, double *centers_out,
                     int32_t *labels_out, double *inertia_out, int64_t *n_iter_out);
/* model.fit(X) (S2C:800): Baum-Welch from startprob (2, never re-estimated), means / covars (2 x D) and transmat
 * (2 x 2, row-major), all updated in place.  logprob_out[i] = log-likelihood of iteration i under the parameters before
 * its M-step; it stops after iteration i when logprob[i] - logprob[i-1] < tol, or after n_iter; *n_done_out =
 * iterations run. */
int hicmi_hmm_fit(hicmi_ctx *ctx, const double *startprob, double *means, double *covars, double *transmat,
                  int64_t n_iter, double tol, double *logprob_out, int64_t *n_done_out);
/* model.predict(X) (S2C:801): Viterbi under the given parameters, ties to state 0.  states_out: T int32. */
int hicmi_hmm_decode(hicmi_ctx *ctx, const double *startprob, const double *means, const double *covars,
                     const double *transmat, int32_t *states_out);
/* Many k-means problems per call: the restarts of many fits (the reference fits one model at a time, S2C:796-801; a
 * parameter sweep fits many - DESIGN.md section 9c).
 * Observation slots: X matrices kept side by side in the context, each with its own T, built width and leading
 * dimension.  hicmi_hmm_load_obs_slot builds slot `slot` as hicmi_hmm_load_obs does (and sizes the work areas of every
 * call above for it); hicmi_hmm_use_obs makes a built slot the X of the single-problem calls above (col_stats, kmeans,
 * fit, decode, get_obs, set_width, dist2).  hicmi_hmm_load_obs and hicmi_hmm_set_obs build slot 0 and select it.
 * A problem is a (slots[p], widths[p]) view: columns [0, widths[p]) of that slot's X, 1 <= widths[p] <= its built width.
 * hicmi_hmm_dist2_multi: for problem p, nrows[p] (1 or 2) rows rows[2p], rows[2p + 1] of its view; out holds, problem
 * after problem, the nrows[p] x T_p distances hicmi_hmm_dist2 gives on that view, bit for bit.
 * hicmi_hmm_kmeans_multi: Lloyd from the rows rows[2p], rows[2p + 1] of its view (copied on the device) with max_iter[p]
 * and tol[p], all problems in lock step; the stop rule is evaluated per problem on the device, the host reads a done
 * count every few steps (HICMI_HMM_POLL, default 8; it changes no result).  centers_out holds, problem after problem,
 * the 2 x D_p centers; inertia_out[p], n_iter_out[p].  Every output equals hicmi_hmm_kmeans on that view from those
 * rows, bit for bit.
 * 1 <= n_prob <= HICMI_HMM_MAX_PROBLEMS, else HICMI_EINVAL (callers split larger batches). */
#define HICMI_HMM_MAX_SLOTS 16
#define HICMI_HMM_MAX_PROBLEMS 256
int hicmi_hmm_load_obs_slot(hicmi_ctx *ctx, int64_t slot, const int32_t *order, int64_t n, int64_t c, int64_t p);
int hicmi_hmm_use_obs(hicmi_ctx *ctx, int64_t slot);
int hicmi_hmm_dist2_multi(hicmi_ctx *ctx, int64_t n_prob, const int64_t *slots, const int64_t *widths, const int64_t *nrows,
                          const int64_t *rows, double *out);
int hicmi_hmm_kmeans_multi(hicmi_ctx *ctx, int64_t n_prob, const int64_t *slots, const int64_t *widths, const int64_t *rows,
                           const int64_t *max_iter, const double *tol, double *centers_out, double *inertia_out,
                           int64_t *n_iter_out);

/* ---- Part 1: Louvain tail (modularity > 0, S2C:239-349) ---------------------------------------------
 * modularity_remaining_data (S2C:263-349) partitions the bins after the last cut index with the best of louvainRounds
 * randomised Louvain runs (S2C:239-262), restated with a seeded generator in modularity.py.  These entry points run
 * level 0 of modularity.best_partition for all rounds on the device; the host keeps levels >= 1.
 * The graph A (m x m, m <= 16384) lives in the context.
 *
 * hicmi_louvain_graph: A = graph_weights(log_transform(similarity tail)) (modularity.py:32-37, 214-220; S2C:285-297):
 * A[i][j] = log10(sim + 1) (0 where sim == 0) of row rows[max(i, j)] and column rows[min(i, j)] of the similarity matrix
 * (S2C:149).  Needs hicmi_row_sums.  Both graph calls also compute _Status's total_weight and gdegrees (modularity.py:43-50)
 * with NumPy's pairwise sums.
 * hicmi_louvain_set_graph / hicmi_louvain_get_graph: an arbitrary symmetric A in; A, gdegrees (m) and total_weight out
 * (each output may be NULL). */
int hicmi_louvain_graph(hicmi_ctx *ctx, const int32_t *rows, int64_t m);
int hicmi_louvain_set_graph(hicmi_ctx *ctx, const double *A, int64_t m);
int hicmi_louvain_get_graph(hicmi_ctx *ctx, double *A_out, double *gdegrees_out, double *total_weight_out);
/* modularity._one_level(_Status(A), rng) (modularity.py:65-112) for `rounds` independent generators, one workgroup each,
 * bit for bit.  states_in / states_out: 6 uint64 per round - numpy PCG64 state low, high 64 bits, inc low, high,
 * has_uint32, uinteger (rng.bit_generator.state).  node2com_out, degrees_out, internals_out: rounds x m (the _Status
 * after level 0).  info_out: 4 int32 per round - passes, tie replays, passes whose gain was within 1e-12 of the 1e-7
 * threshold, 0.  More than 1024 rounds: HICMI_EINVAL; m > 16384: HICMI_EUNSUPPORTED (at the graph call). */
int hicmi_louvain_level0(hicmi_ctx *ctx, int64_t rounds, const uint64_t *states_in, int32_t *node2com_out,
                         uint64_t *states_out, int32_t *info_out, double *degrees_out, double *internals_out);
/* modularity._induced(A, part) (modularity.py:124-134): the k x k community graph of part (m labels in [0, k)).
 * hicmi_louvain_modularity: modularity.modularity(part, A) (modularity.py:165-180) of `rounds` partitions (rounds x m,
 * labels in [0, m)).  m must be the graph's.  Both sum in a fixed order of their own: within 1e-12 of the host's BLAS
 * products. */
int hicmi_louvain_induced(hicmi_ctx *ctx, const int32_t *part, int64_t m, int64_t k, double *out);
int hicmi_louvain_modularity(hicmi_ctx *ctx, const int32_t *parts, int64_t rounds, int64_t m, double *q_out);

/* ---- Part 1: group support ----------------------------------------------------
 * assessChromosomeClustering (S2C:1001-1077) assigns a scaffold to a chromosome group by a vote of its bins; this entry
 * point extends that call site with the evidence of the contacts: how densely every bin and every scaffold touches
 * every group.  On the context's contact matrix as it stands (uploaded, adopted with ld > n, or compacted; n bins):
 * grp[i] in -1 .. n_groups - 1 (the group of bin i, -1: none) and scaf[i] in 0 .. n_scaffolds - 1 (a dense scaffold id)
 * for every bin; a value outside those ranges: HICMI_EINVAL.
 *   bin_sums_out[i * n_groups + g]      = sum of M[j][i] over the rows j with grp[j] == g and scaf[j] != scaf[i]
 *                                         (n x n_groups, may be NULL): a scaffold's own bins never vote for it;
 *   scaffold_sums_out[s * n_groups + g] = sum of that over the bins i of scaffold s (n_scaffolds x n_groups).
 * The order of every sum is fixed, so the tables are reproducible to the last bit: the members of g by ascending row in
 * chunks of 64, each chunk left to right from 0.0, the chunk sums left to right; a scaffold's bins left to right in
 * matrix order.  Every grouped row is read once (k_gs_partial, k_gs_reduce); HICMI_GROUP_SUPPORT_PLAIN=1 in the
 * environment takes the one-thread-per-(column, group) kernel instead, with the same bits.
 * Device scratch: (grouped rows / 64 + n_groups) x n partials and the two tables; n_groups <= 65536. */
int hicmi_group_sums(hicmi_ctx *ctx, const int32_t *grp, const int32_t *scaf, int64_t n_groups, int64_t n_scaffolds,
                     double *bin_sums_out, double *scaffold_sums_out);

/* ---- Part 2: junction support ---------------------------------------------------
 * orderGenome.py's chromosome loop (OG:608-612) orders every chromosome group on its own; nothing there looks from one
 * group at another, or asks whether the two sides of a scaffold boundary belong together.  This entry point extends that
 * call site: on the context's contact matrix M as it stands (uploaded fp64, fp32 widened, adopted with ld > n, or
 * compacted; n bins), bins[0 .. n_listed) is the bin order of every ordered chromosome, one after the other, as matrix
 * indices in [0, n) - uploaded once per call - and rec holds six values per record: startA, stepA, lenA, startB, stepB,
 * lenB.  A side is read outwards from a junction: its entry k is bins[start + k * step], step = +1 or -1, entry 0
 * touching the junction.
 *   sums_out[r] = sum over a < lenA, b < lenB of M[A_a][B_b] * (1.0 / (a + b + 1))
 * The weights come from a table of 1.0 / d the library builds on the host (IEEE division) and uploads; the kernels do not
 * divide, and each product is rounded before it is added.  The order of every sum is fixed by (lenA, lenB) alone, so two
 * calls give the same bits: A's rows in slabs of 64, a slab's rows x lenB elements dealt row-major to 256 lanes, the lane
 * sums added as a fixed tree, the slab sums left to right (k_junctions_partial, k_junctions_reduce: no atomics, no
 * dynamic LDS, nothing staged per record).  HICMI_JUNCTIONS_PLAIN=1 in the environment takes one thread per record with
 * a serial double loop instead - the definition taken literally, the A/B path; it differs in rounding only.
 * HICMI_EINVAL when no matrix is set, a length is below 1, a step is not +1 or -1, a side runs outside bins, or a bin is
 * outside [0, n); HICMI_EUNSUPPORTED above 2^31 - 1 workgroups (the sum over the records of ceil(lenA / 64)).  Either is
 * returned before anything is launched, with the context unchanged.  n_rec = 0: nothing to do.
 * Device scratch: the records, bins, the weights and one double per workgroup and per record. */
int hicmi_junction_sums(hicmi_ctx *ctx, const int32_t *bins, int64_t n_listed, const int64_t *rec, int64_t n_rec,
                        double *sums_out);

/* ---- Part 0: ICE balancing of a raw map ----------------------------------------
 * Replaces HiC-Pro's `ice` step (ice --filter_low_counts_perc 0.02 --filter_high_counts_perc 0 --max_iter 100 --eps 0.1
 * --remove-all-zeros-loci --output-bias 1; iced.normalization.ICE_normalization and iced.filter), which the reference
 * expects to have run before its loaders (S2C:35-98 read its two output files).  Both calls rewrite the context's OWN
 * contact matrix (uploaded or compacted; leading dimension honoured): a matrix adopted with hicmi_set_contacts_device is
 * the caller's and is refused with HICMI_ESTATE, untouched.  Row sums, rank matrix and Part 2 selection of the context
 * are invalidated.
 *
 * hicmi_ice_mask_rows replaces iced.filter's zeroing of the filtered loci: rows and columns i with mask[i] != 0 of the
 * resident matrix become 0 (n = the matrix size).  The row weights the mask rules need come from hicmi_row_sums. */
int hicmi_ice_mask_rows(hicmi_ctx *ctx, const uint8_t *mask, int64_t n);
/* hicmi_ice_balance replaces iced.normalization.ICE_normalization (HiC-Pro's `ice` proper): with X = C (masked rows and
 * columns zeroed first; mask may be NULL), bias = 1, mean0 = sum X / n^2, for it = 0 .. max_iter - 1:
 *   s_i = sum_j X_ij;  d_i = s_i / mean(s over s != 0), 1 where s_i == 0;  bias_i *= d_i;  X_ij /= d_i d_j;
 *   c = (sum X / n^2) / mean0;  bias *= sqrt(c);  X /= c;  stop if it > 0 and sum_i |bias_prev_i - bias_i| < eps.
 * The resident matrix becomes X (exactly symmetric, masked rows and columns exactly 0).  bias_out (n, may be NULL): the
 * biases, NaN for masked bins; *iters_out: iterations run (max_iter when it did not converge: not an error);
 * *delta_out: the last sum |bias_prev - bias| (NaN when fewer than two iterations ran).
 * By default X is never formed during the loop: with u = 1 / bias, s_i = u_i sum_j C_ij u_j is one read-only pass over
 * the raw map per iteration, every sum in a fixed order (two calls give the same bits), and X_ij = C_ij (u_i u_j) once at
 * the end.  HICMI_ICE_INPLACE=1 in the environment rescales the matrix in place every iteration instead (the A/B). */
int hicmi_ice_balance(hicmi_ctx *ctx, const uint8_t *mask, int64_t max_iter, double eps, double *bias_out,
                      int64_t *iters_out, double *delta_out);
/* Copy rows [row0, row0+nrows) of the context's contact matrix to the host, n doubles per row (the balanced map for the
 * writer of HiC-Pro's *_iced.matrix file; tests). */
int hicmi_get_contact_rows(hicmi_ctx *ctx, int64_t row0, int64_t nrows, double *out);

/* ---- timing ----------------------------------------------------------------------------------
 * Accumulated device time (HIP events on the context stream) per kernel family since the last
 * reset, for bench.py's roofline object.  names_out: caller buffer receiving ';'-separated names;
 * ms_out / launches_out / bytes_out: one entry per name (algorithmic bytes as defined in DESIGN.md).
 * hicmi_timing_enable: 0 = off, 1 = every family, 2 = only the Part 1 families that are launched a few times
 * per map: row_sums, build_w, nnchain, sort_rows, rank_invert, and the three of the pre-sort path - presort_rows,
 * rank_relabel, rank_rows_tied.  (presort_rows and the rank_invert behind it are recorded on the pre-sort's second
 * stream, beside the nn-chain: their ms overlap the chain's.)  Launches and bytes are counted in every mode; ms is
 * 0 for a family the mode does not time.  p2_window_G_flops is a pure counter: its "bytes" are the flops of the
 * window tables' GEMM, its ms is always 0.  An event pair whose elapsed time cannot be read is an error
 * (HICMI_EHIP) of the call that collects it - reset, enable or get - never a smaller sum. */
int hicmi_timing_reset(hicmi_ctx *ctx);
int hicmi_timing_enable(hicmi_ctx *ctx, int on);
int hicmi_timing_get(hicmi_ctx *ctx, char *names_out, int64_t names_cap, double *ms_out,
                     int64_t *launches_out, double *bytes_out, int64_t cap, int64_t *count_out);

#ifdef __cplusplus
}
#endif
#endif /* HICMI_H */
