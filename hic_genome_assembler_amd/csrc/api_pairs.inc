// api_pairs.inc - the resident pair store (DESIGN.md 9r), seat support (9s) and the end-link graph (9t) on it, a part of api.hip that is
// included there after the ends and the anchor calls it builds on.  The store lives in buffers of its own: the context's matrix state and open map, span, ends
// and anchor builds are never touched by hicmi_pairs_* (the staging of a chunk, d_map_chunk, holds nothing between calls).
// the rows of hicmi_links_resident (DESIGN.md 9t) belong to the store they were counted from and go with it
static void links_abandon(hicmi_ctx* c)
{
    c->d_links_table.reset(); c->d_links_recs.reset(); c->d_links_size.reset();
    c->links_lo.clear(); c->links_hi.clear(); c->links_counts.clear();
    c->links_ready = false;
}

static void pairs_abandon(hicmi_ctx* c)
{
    links_abandon(c);
    c->d_pairs_scaf_a.reset(); c->d_pairs_pos_a.reset(); c->d_pairs_scaf_b.reset(); c->d_pairs_pos_b.reset();
    c->d_pairs_intra.reset(); c->d_pairs_work.reset();
    c->pairs_size.clear();
    c->pairs_len = 0;
}

// HICMI_PAIRS_PLAIN: "1" one bump of the length per kept pair, "0" the stable compaction, anything else the default; read per call
constexpr bool kPairsPlainByDefault = false;
static bool pairs_plain()
{
    return plain_switch(getenv("HICMI_PAIRS_PLAIN"), kPairsPlainByDefault);
}

// HICMI_PAIRS_FIRST_PAIRS, the first capacity of a store; read per begin
static int pairs_first_setting(int64_t* out)
{
    return setting_in_range("HICMI_PAIRS_FIRST_PAIRS", getenv("HICMI_PAIRS_FIRST_PAIRS"), 31, PAIRS_FIRST_PAIRS, out);
}

static unsigned long long* pairs_length(hicmi_ctx* c) { return c->d_pairs_intra + c->pairs_size.size(); }

// room for `need` pairs: the capacity at least doubles, and the pairs in use move by device-to-device copy
static int pairs_reserve(hicmi_ctx* c, int64_t need)
{
    if (need <= c->d_pairs_scaf_a.capacity()) return HICMI_OK;
    const int64_t cap = std::max(need, 2 * c->d_pairs_scaf_a.capacity());
    DevBuf<int32_t> scaf_a, scaf_b;
    DevBuf<int64_t> pos_a, pos_b;
    int rc = ensure_all(scaf_a, cap, pos_a, cap, scaf_b, cap, pos_b, cap);
    if (rc) return rc;
    const size_t n = (size_t)c->pairs_len;
    if (n) {
        HIPCHK(hipMemcpyAsync(scaf_a, c->d_pairs_scaf_a, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(pos_a, c->d_pairs_pos_a, sizeof(int64_t) * n, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(scaf_b, c->d_pairs_scaf_b, sizeof(int32_t) * n, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(pos_b, c->d_pairs_pos_b, sizeof(int64_t) * n, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));                      // the old arrays are read no more
    c->d_pairs_scaf_a = std::move(scaf_a); c->d_pairs_pos_a = std::move(pos_a);
    c->d_pairs_scaf_b = std::move(scaf_b); c->d_pairs_pos_b = std::move(pos_b);
    return HICMI_OK;
}

// an empty store and the zeroed intra array, all or nothing
static int pairs_open(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf)
{
    if (!c || !scaf_size || n_scaf < 1 || n_scaf > INT_MAX / 2) return fail(HICMI_EINVAL, "bad arguments");
    if (c->d_pairs_intra) return fail(HICMI_EINVAL, "the context already has a pair store: hicmi_pairs_drop first");
    for (int64_t s = 0; s < n_scaf; s++)
        if (scaf_size[s] < 0) return fail(HICMI_EINVAL, "scaffold %lld has a negative size", (long long)s);
    int64_t first = 0;
    int rc = pairs_first_setting(&first);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(c->pin_pairs_len.reserve(1));
    rc = ensure_all(c->d_pairs_intra, n_scaf + 1, c->d_pairs_scaf_a, first, c->d_pairs_pos_a, first, c->d_pairs_scaf_b, first,
                    c->d_pairs_pos_b, first);
    if (rc) { pairs_abandon(c); return rc; }
    hipError_t e = hipMemsetAsync(c->d_pairs_intra, 0, sizeof(uint64_t) * (size_t)(n_scaf + 1), c->stream);
    if (e == hipSuccess) e = sync_stream(c);
    if (e != hipSuccess) { pairs_abandon(c); return fail(HICMI_EHIP, "hipMemsetAsync: %s", hipGetErrorString(e)); }
    c->pairs_size.assign(scaf_size, scaf_size + n_scaf);
    c->pairs_len = 0;
    *c->pin_pairs_len.get() = 0ull;
    return HICMI_OK;
}

// a chunk on the device into the store; the length is on its way back into pin_pairs_len when this returns
static int pairs_keep_chunk(hicmi_ctx* c, const MapChunk& d, int64_t n, bool plain)
{
    int rc = pairs_reserve(c, c->pairs_len + n);
    if (!rc && !plain) rc = ensure(c->d_pairs_work, pairs_keep_blocks(n));
    if (rc) return rc;
    PairStore store;
    store.scaf_a = c->d_pairs_scaf_a; store.pos_a = c->d_pairs_pos_a; store.scaf_b = c->d_pairs_scaf_b; store.pos_b = c->d_pairs_pos_b;
    store.cap = c->d_pairs_scaf_a.capacity();                     // the four arrays are reserved alike
    launch_pairs_keep(d.scaf_a, d.pos_a, d.scaf_b, d.pos_b, n, (int64_t)c->pairs_size.size(), store, pairs_length(c), c->d_pairs_intra,
                      c->d_pairs_work, plain, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->pin_pairs_len, pairs_length(c), sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    return HICMI_OK;
}

int hicmi_pairs_begin(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf)
{
    return pairs_open(c, scaf_size, n_scaf);
}

int hicmi_pairs_add(hicmi_ctx* c, const int32_t* scaf_a, const int64_t* pos_a, const int32_t* scaf_b, const int64_t* pos_b, int64_t n)
{
    if (!c || n < 0 || (n > 0 && (!scaf_a || !pos_a || !scaf_b || !pos_b))) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->d_pairs_intra) return fail(HICMI_EINVAL, "hicmi_pairs_add without hicmi_pairs_begin");
    int rc_pairs = check_pairs(scaf_a, pos_a, scaf_b, pos_b, n, c->pairs_size.data(), (int64_t)c->pairs_size.size(), nullptr, nullptr);
    if (rc_pairs) return rc_pairs;
    if (n == 0) return HICMI_OK;
    c->links_ready = false;                                        // rows counted before these pairs are not the store's any more
    HIPCHK(hipSetDevice(c->device));
    // a HIP error from here on gives the store up: what was kept so far cannot be told
    MapChunk k;
    int rc = stage_chunk(c, scaf_a, pos_a, scaf_b, pos_b, n, &k);
    if (!rc) rc = pairs_keep_chunk(c, k, n, pairs_plain());
    if (!rc) {
        const hipError_t e = sync_stream(c);
        if (e != hipSuccess) rc = fail(HICMI_EHIP, "keeping a chunk of pairs: %s", hipGetErrorString(e));
    }
    if (rc) { pairs_abandon(c); return rc; }
    c->pairs_len = (int64_t)*c->pin_pairs_len.get();
    return HICMI_OK;
}

// begin and every pair of the file in one pass with pair_file_pass; a store is left only when the whole
// file is down
int hicmi_pairs_file(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names, const int64_t* scaf_size,
                     hicmi_ctx* c, int threads, int64_t* stats5)
{
    if (!path || !names_blob || !name_off || !scaf_size || !c || !stats5 || n_names < 1) return fail(HICMI_EINVAL, "bad arguments");
    int64_t chunk_pairs = 0;
    int rc = chunk_pairs_setting(&chunk_pairs);
    if (rc) return rc;
    rc = pairs_open(c, scaf_size, n_names);
    if (rc) return rc;
    struct OpenPairs { hicmi_ctx* c; bool keep = false; ~OpenPairs() { if (!keep) pairs_abandon(c); } } own{c};   // given up on every error path
    const bool plain = pairs_plain();
    int64_t stats[5] = {0, 0, 0, 0, 0};
    rc = pair_file_pass(path, names_blob, name_off, n_names, scaf_size, c, threads, chunk_pairs, stats, "keeping a chunk of pairs",
                        [&](const MapChunk& d, int64_t n) -> int {
                            c->pairs_len = (int64_t)*c->pin_pairs_len.get();   // the chunk before is done: its length is down
                            return pairs_keep_chunk(c, d, n, plain);
                        });
    if (rc) return rc;
    c->pairs_len = (int64_t)*c->pin_pairs_len.get();
    own.keep = true;
    for (int k = 0; k < 5; k++) stats5[k] = stats[k];
    return HICMI_OK;
}

int hicmi_pairs_info(hicmi_ctx* c, int64_t* n_kept_out, uint64_t* n_intra_out, uint64_t* intra_out)
{
    if (!c || !n_kept_out || !n_intra_out) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->d_pairs_intra) return fail(HICMI_EINVAL, "hicmi_pairs_info without a pair store");
    HIPCHK(hipSetDevice(c->device));
    std::vector<uint64_t> intra(c->pairs_size.size());
    int rc = download(c, intra.data(), c->d_pairs_intra, sizeof(uint64_t) * intra.size());
    if (rc) return rc;
    uint64_t total = 0;
    for (const uint64_t v : intra) total += v;
    *n_kept_out = c->pairs_len; *n_intra_out = total;
    if (intra_out) memcpy(intra_out, intra.data(), sizeof(uint64_t) * intra.size());
    return HICMI_OK;
}

int hicmi_pairs_fetch(hicmi_ctx* c, int32_t* scaf_a, int64_t* pos_a, int32_t* scaf_b, int64_t* pos_b)
{
    if (!c) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->d_pairs_intra) return fail(HICMI_EINVAL, "hicmi_pairs_fetch without a pair store");
    const size_t n = (size_t)c->pairs_len;
    if (n == 0) return HICMI_OK;
    if (!scaf_a || !pos_a || !scaf_b || !pos_b) return fail(HICMI_EINVAL, "bad arguments");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(scaf_a, c->d_pairs_scaf_a, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pos_a, c->d_pairs_pos_a, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(scaf_b, c->d_pairs_scaf_b, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(pos_b, c->d_pairs_pos_b, sizeof(int64_t) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(sync_stream(c));
    return HICMI_OK;
}

int hicmi_pairs_drop(hicmi_ctx* c)
{
    if (!c) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->d_pairs_intra) return fail(HICMI_EINVAL, "hicmi_pairs_drop without a pair store");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(sync_stream(c));
    pairs_abandon(c);
    return HICMI_OK;
}

// what a resident call asks of the store before anything else: there is one, and it was loaded for these scaffolds
static int pairs_resident_check(const hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const char* call)
{
    if (!c->d_pairs_intra) return fail(HICMI_EINVAL, "%s without a pair store", call);
    if (!scaf_size || n_scaf != (int64_t)c->pairs_size.size() || memcmp(scaf_size, c->pairs_size.data(), sizeof(int64_t) * (size_t)n_scaf))
        return fail(HICMI_EINVAL, "%s: the scaffold sizes are not the ones the pair store was loaded with", call);
    return HICMI_OK;
}

// hicmi_ends_file with the store in place of the file: the count kernel over the kept pairs, then the intra pairs by their sums
int hicmi_ends_resident(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                        const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, int64_t window, int64_t reach,
                        uint64_t* table_out, uint64_t* counters6_out, int32_t* rank_out, int64_t* n_placed_out)
{
    if (!c || !table_out || !counters6_out || !rank_out || !n_placed_out) return fail(HICMI_EINVAL, "bad arguments");
    int rc = pairs_resident_check(c, scaf_size, n_scaf, "hicmi_ends_resident");
    if (rc) return rc;
    if (c->ends_table) return fail(HICMI_EINVAL, "hicmi_ends_resident while an ends build is open");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    EndsRanks ranks;
    rc = ends_number(scaf_size, n_scaf, lift, window, reach, &ranks);
    if (rc) return rc;
    rc = ends_open(c, scaf_size, n_scaf, lift, window, reach, ranks);
    if (rc) return rc;
    struct OpenEnds { hicmi_ctx* c; bool keep = false; ~OpenEnds() { if (!keep) ends_abandon(c); } } own{c};   // given up on every error path
    std::vector<uint64_t> intra((size_t)n_scaf);
    rc = download(c, intra.data(), c->d_pairs_intra, sizeof(uint64_t) * intra.size());
    if (rc) return rc;
    launch_ends_count(c->d_pairs_scaf_a, c->d_pairs_pos_a, c->d_pairs_scaf_b, c->d_pairs_pos_b, c->pairs_len, c->ends_lift, c->ends_grid,
                      c->ends_cells, c->ends_table, c->ends_table + c->ends_cells, ends_plain(), c->stream);
    HIPCHK(hipGetLastError());
    // the table comes down into memory of the library's first: an error after it leaves every output as it was
    std::vector<uint64_t> table((size_t)c->ends_cells);
    uint64_t counters[ENDS_COUNTERS];
    own.keep = true;                                               // ends_close closes the build, whatever it returns
    rc = ends_close(c, table.data(), counters);
    if (rc) return rc;
    pairs_add_intra_ends(intra.data(), lift_seq, n_scaf, counters);
    memcpy(table_out, table.data(), sizeof(uint64_t) * table.size());
    memcpy(counters6_out, counters, sizeof(counters));
    memcpy(rank_out, ranks.rank.data(), sizeof(int32_t) * (size_t)n_scaf);
    *n_placed_out = ranks.n_placed;
    return HICMI_OK;
}

// hicmi_anchor_file with the store in place of the file
int hicmi_anchor_resident(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                          const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, const int32_t* target, int64_t window,
                          uint64_t* table_out, uint64_t* counters6_out, int64_t* first_out, int64_t* n_table_out)
{
    if (!c || !table_out || !counters6_out || !first_out || !n_table_out) return fail(HICMI_EINVAL, "bad arguments");
    int rc = pairs_resident_check(c, scaf_size, n_scaf, "hicmi_anchor_resident");
    if (rc) return rc;
    if (c->anchor_table) return fail(HICMI_EINVAL, "hicmi_anchor_resident while an anchor build is open");
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    AnchorBlocks blocks;
    rc = anchor_number(scaf_size, n_scaf, lift, target, window, &blocks);
    if (rc) return rc;
    rc = anchor_open(c, scaf_size, n_scaf, lift, target, window, blocks);
    if (rc) return rc;
    struct OpenAnchor { hicmi_ctx* c; bool keep = false; ~OpenAnchor() { if (!keep) anchor_abandon(c); } } own{c};   // given up on every error path
    std::vector<uint64_t> intra((size_t)n_scaf);
    rc = download(c, intra.data(), c->d_pairs_intra, sizeof(uint64_t) * intra.size());
    if (rc) return rc;
    launch_anchor_count(c->d_pairs_scaf_a, c->d_pairs_pos_a, c->d_pairs_scaf_b, c->d_pairs_pos_b, c->pairs_len, c->anchor_lift,
                        c->anchor_grid, c->anchor_cells, c->anchor_table, c->anchor_table + c->anchor_cells, anchor_plain(), c->stream);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> table((size_t)c->anchor_cells);
    uint64_t counters[ANCHOR_COUNTERS];
    own.keep = true;                                               // anchor_close closes the build, whatever it returns
    rc = anchor_close(c, table.data(), counters);
    if (rc) return rc;
    pairs_add_intra_anchor(intra.data(), lift_seq, n_scaf, counters);
    memcpy(table_out, table.data(), sizeof(uint64_t) * table.size());
    memcpy(counters6_out, counters, sizeof(counters));
    memcpy(first_out, blocks.first.data(), sizeof(int64_t) * (size_t)n_scaf);
    *n_table_out = blocks.n_table;
    return HICMI_OK;
}

// ---- seat support (DESIGN.md 9s): every placed scaffold against the chromosomes and the gaps of its own, in one pass --------
static void seats_abandon(hicmi_ctx* c)
{
    c->seats_table.reset(); c->d_seats_lift.reset(); c->d_seats_first.reset(); c->d_seats_rank.reset();
}

// HICMI_SEATS_PLAIN: "1" up to four atomic adds per pair, "0" the combining kernel, anything else the default; read per call
constexpr bool kSeatsPlainByDefault = false;
static bool seats_plain()
{
    return plain_switch(getenv("HICMI_SEATS_PLAIN"), kSeatsPlainByDefault);
}

// What hicmi_anchor_resident would count in both of its modes if one placed scaffold alone were taken out of the ordering,
// for every placed scaffold at once.  The buffers live for this call only and are closed on every path.
int hicmi_seats_resident(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                         const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, int64_t window, uint64_t* table_out,
                         uint64_t* counters5_out, int64_t* first_out, int64_t* n_table_out)
{
    if (!c || !table_out || !counters5_out || !first_out || !n_table_out) return fail(HICMI_EINVAL, "bad arguments");
    int rc = pairs_resident_check(c, scaf_size, n_scaf, "hicmi_seats_resident");
    if (rc) return rc;
    if (window < 1) return fail(HICMI_EINVAL, "window %lld is below 1", (long long)window);
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    rc = lift_check(scaf_size, n_scaf, lift);
    if (rc) return rc;
    std::vector<int32_t> rank((size_t)n_scaf);
    std::vector<int64_t> blocks((size_t)(n_scaf + n_seq + 1));        // [first n_scaf][seq_first n_seq + 1], as on the device
    int64_t* first = blocks.data();
    int64_t* seq_first = first + n_scaf;
    if (ends_number_ranks(scaf_size, n_scaf, lift_seq, lift_off, n_seq, 1, rank.data(), seq_first) < 0)
        return fail(HICMI_EUNSUPPORTED, "more than %lld placed scaffolds", (long long)(ENDS_MAX_TABLE / 4));
    const int64_t m = seats_number_blocks(scaf_size, n_scaf, lift_seq, n_seq, seq_first, first);
    if (m < 0) return fail(HICMI_EUNSUPPORTED, "the placed scaffolds need a table of more than %lld counters", (long long)SEATS_MAX_TABLE);
    if (m < 1) return fail(HICMI_EINVAL, "no scaffold with a base is placed");
    HIPCHK(hipSetDevice(c->device));
    struct OpenSeats { hicmi_ctx* c; ~OpenSeats() { seats_abandon(c); } } own{c};            // closed on every path
    rc = ensure_all(c->seats_table, m + SEATS_COUNTERS, c->d_seats_first, n_scaf + n_seq + 1, c->d_seats_rank, n_scaf, c->d_seats_lift,
                    21 * n_scaf);
    if (rc) return rc;
    LiftTables d_lift;
    rc = upload(c, c->d_seats_first, blocks.data(), sizeof(int64_t) * blocks.size());
    if (!rc) rc = upload(c, c->d_seats_rank, rank.data(), sizeof(int32_t) * (size_t)n_scaf);
    if (!rc) rc = lift_upload(c, c->d_seats_lift, scaf_size, n_scaf, lift, &d_lift);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(c->seats_table, 0, sizeof(uint64_t) * (size_t)(m + SEATS_COUNTERS), c->stream));
    HIPCHK(sync_stream(c));                                        // the tables have left the upload arena
    std::vector<uint64_t> intra((size_t)n_scaf);
    rc = download(c, intra.data(), c->d_pairs_intra, sizeof(uint64_t) * intra.size());
    if (rc) return rc;
    SeatsGrid grid;
    grid.first = c->d_seats_first; grid.seq_first = c->d_seats_first + n_scaf; grid.rank = c->d_seats_rank; grid.window = window;
    launch_seats_count(c->d_pairs_scaf_a, c->d_pairs_pos_a, c->d_pairs_scaf_b, c->d_pairs_pos_b, c->pairs_len, d_lift, grid, m,
                       c->seats_table, c->seats_table + m, seats_plain(), c->stream);
    HIPCHK(hipGetLastError());
    // the table comes down into memory of the library's first: an error after it leaves every output as it was
    std::vector<uint64_t> table((size_t)m);
    uint64_t counters[SEATS_COUNTERS];
    rc = download_table(c, c->seats_table, m, SEATS_COUNTERS, table.data(), counters);
    if (rc) return rc;
    seats_add_intra(intra.data(), lift_seq, n_scaf, counters);
    memcpy(table_out, table.data(), sizeof(uint64_t) * table.size());
    memcpy(counters5_out, counters, sizeof(counters));
    memcpy(first_out, first, sizeof(int64_t) * (size_t)n_scaf);
    *n_table_out = m;
    return HICMI_OK;
}

// ---- the end-link graph of all scaffolds (DESIGN.md 9t): which scaffold ends are linked to which, before any ordering ------
// HICMI_LINKS_PLAIN: "1" one find-or-insert per pair, "0" the combining kernel, anything else the default; read per call
constexpr bool kLinksPlainByDefault = false;
static bool links_plain()
{
    return plain_switch(getenv("HICMI_LINKS_PLAIN"), kLinksPlainByDefault);
}

// One pass over the store into a find-or-insert table sized for every key the call can see, the used slots compacted on
// the device, sorted by key on the host (a radix sort, links.h: the records are few next to the pairs, DESIGN.md 9t) and merged into
// one row per scaffold pair.  The rows stay on the context until the store goes; the device buffers stay with them, so a
// second call on the same store allocates nothing.
int hicmi_links_resident(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, int64_t window, int64_t* n_rows_out,
                         uint64_t* counters2_out)
{
    if (!c || !n_rows_out || !counters2_out) return fail(HICMI_EINVAL, "bad arguments");
    if (n_scaf > LINKS_MAX_SCAF) return fail(HICMI_EUNSUPPORTED, "%lld scaffolds, more than the %lld a link key has room for",
                                             (long long)n_scaf, (long long)LINKS_MAX_SCAF);
    int rc = pairs_resident_check(c, scaf_size, n_scaf, "hicmi_links_resident");
    if (rc) return rc;
    if (window < 1) return fail(HICMI_EINVAL, "window %lld is below 1", (long long)window);
    LinksTable T;
    T.cap = links_capacity(c->pairs_len, n_scaf, &T.bits);
    if (T.cap > LINKS_MAX_SLOTS)
        return fail(HICMI_EUNSUPPORTED, "the link table needs %lld slots, more than the %lld a call can have", (long long)T.cap,
                    (long long)LINKS_MAX_SLOTS);
    const int64_t most = links_most_keys(c->pairs_len, n_scaf);
    HIPCHK(hipSetDevice(c->device));
    rc = ensure_all(c->d_links_table, 2 * T.cap + LINKS_EXTRAS, c->d_links_recs, 2 * most, c->d_links_size, n_scaf);
    if (rc) { links_abandon(c); return rc; }
    T.keys = c->d_links_table; T.counts = T.keys + T.cap; T.extras = T.counts + T.cap;
    unsigned long long* rec_key = c->d_links_recs;
    unsigned long long* rec_cnt = rec_key + most;
    rc = upload(c, c->d_links_size, scaf_size, sizeof(int64_t) * (size_t)n_scaf);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(T.keys, 0xFF, sizeof(uint64_t) * (size_t)T.cap, c->stream));
    HIPCHK(hipMemsetAsync(T.counts, 0, sizeof(uint64_t) * (size_t)(T.cap + LINKS_EXTRAS), c->stream));
    if (c->pairs_len > 0) {
        launch_links_count(c->d_pairs_scaf_a, c->d_pairs_pos_a, c->d_pairs_scaf_b, c->d_pairs_pos_b, c->pairs_len, c->d_links_size, n_scaf,
                           window, T, links_plain(), c->stream);
        HIPCHK(hipGetLastError());
        launch_links_compact(T, rec_key, rec_cnt, most, c->stream);
        HIPCHK(hipGetLastError());
    }
    uint64_t extras[LINKS_EXTRAS];
    rc = download(c, extras, T.extras, sizeof(extras));           // synchronises: the sizes have left the upload arena
    if (rc) return rc;
    if (extras[LINKS_FLAG])
        return fail(HICMI_EHIP, "the link table of %lld slots ran full (flag %llu): the store holds pairs the call did not expect",
                    (long long)T.cap, (unsigned long long)extras[LINKS_FLAG]);
    const int64_t n_rec = (int64_t)extras[LINKS_RECORDS];
    if (n_rec < 0 || n_rec > most) return fail(HICMI_EHIP, "%lld link records where %lld fit", (long long)n_rec, (long long)most);
    // the records come down into memory of the library's first: an error after it leaves every output as it was
    std::vector<uint64_t> key((size_t)n_rec), count((size_t)n_rec);
    if (n_rec) {
        HIPCHK(hipMemcpyAsync(key.data(), rec_key, sizeof(uint64_t) * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(count.data(), rec_cnt, sizeof(uint64_t) * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(sync_stream(c));
    }
    // the slot order is the race's: sorted by key on the host, timed for hicmi_links_info
    const auto t0 = std::chrono::steady_clock::now();
    links_sort_records(key.data(), count.data(), n_rec);
    const double sort_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::vector<int32_t> lo((size_t)n_rec), hi((size_t)n_rec);
    std::vector<uint64_t> counts5((size_t)n_rec * LINKS_COMBOS);
    const int64_t n_rows = links_merge_rows(key.data(), count.data(), n_rec, lo.data(), hi.data(), counts5.data());
    lo.resize((size_t)n_rows); hi.resize((size_t)n_rows); counts5.resize((size_t)n_rows * LINKS_COMBOS);
    c->links_lo = std::move(lo); c->links_hi = std::move(hi); c->links_counts = std::move(counts5);
    c->links_ready = true;
    c->links_records = n_rec; c->links_slots = T.cap; c->links_sort_ms = sort_ms;
    *n_rows_out = n_rows;
    counters2_out[LINKS_LINKED] = extras[LINKS_LINKED];
    counters2_out[LINKS_MIDDLE] = extras[LINKS_MIDDLE];
    return HICMI_OK;
}

int hicmi_links_fetch(hicmi_ctx* c, int32_t* lo, int32_t* hi, uint64_t* counts5)
{
    if (!c) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->links_ready) return fail(HICMI_EINVAL, "hicmi_links_fetch before hicmi_links_resident");
    const size_t n = c->links_lo.size();
    if (n == 0) return HICMI_OK;
    if (!lo || !hi || !counts5) return fail(HICMI_EINVAL, "bad arguments");
    memcpy(lo, c->links_lo.data(), sizeof(int32_t) * n);
    memcpy(hi, c->links_hi.data(), sizeof(int32_t) * n);
    memcpy(counts5, c->links_counts.data(), sizeof(uint64_t) * n * LINKS_COMBOS);
    return HICMI_OK;
}

int hicmi_links_info(hicmi_ctx* c, int64_t* n_records_out, int64_t* n_slots_out, double* sort_ms_out)
{
    if (!c || !n_records_out || !n_slots_out || !sort_ms_out) return fail(HICMI_EINVAL, "bad arguments");
    if (!c->links_ready) return fail(HICMI_EINVAL, "hicmi_links_info before hicmi_links_resident");
    *n_records_out = c->links_records; *n_slots_out = c->links_slots; *sort_ms_out = c->links_sort_ms;
    return HICMI_OK;
}
