// api_links.inc - the end-link graph between the ends of sequences that consist of several scaffolds (DESIGN.md 9u), a part
// of api.hip that is included behind api_pairs.inc: it counts the resident pair store of that file into the table, the
// records and the rows of hicmi_links_resident, which hicmi_links_fetch and hicmi_links_info then answer from.

// One pass over the store, every end lifted onto its sequence first, into a find-or-insert table sized for every key of n_seq
// sequences; from there on as hicmi_links_resident: the used slots compacted on the device, sorted by key on the host and
// merged into one row per sequence pair.  The lift tables and the sequence sizes live on the device for this call only.
int hicmi_links_lifted(hicmi_ctx* c, const int64_t* scaf_size, int64_t n_scaf, const int32_t* lift_seq, const int64_t* lift_off,
                       const uint8_t* lift_rev, const int64_t* seq_size, int64_t n_seq, int64_t window, int64_t* n_rows_out,
                       uint64_t* counters4_out)
{
    if (!c || !n_rows_out || !counters4_out) return fail(HICMI_EINVAL, "bad arguments");
    int rc = pairs_resident_check(c, scaf_size, n_scaf, "hicmi_links_lifted");
    if (rc) return rc;
    if (window < 1) return fail(HICMI_EINVAL, "window %lld is below 1", (long long)window);
    const LiftHost lift{lift_seq, lift_off, lift_rev, seq_size, n_seq};
    rc = lift_check(scaf_size, n_scaf, lift);
    if (rc) return rc;
    if (n_seq > LINKS_MAX_SCAF) return fail(HICMI_EUNSUPPORTED, "%lld sequences, more than the %lld a link key has room for",
                                            (long long)n_seq, (long long)LINKS_MAX_SCAF);
    LinksTable T;
    T.cap = links_capacity(c->pairs_len, n_seq, &T.bits);
    if (T.cap > LINKS_MAX_SLOTS)
        return fail(HICMI_EUNSUPPORTED, "the link table needs %lld slots, more than the %lld a call can have", (long long)T.cap,
                    (long long)LINKS_MAX_SLOTS);
    const int64_t most = links_most_keys(c->pairs_len, n_seq);
    HIPCHK(hipSetDevice(c->device));
    struct OpenLift { hicmi_ctx* c; ~OpenLift() { c->d_links_lift.reset(); c->d_links_seq_size.reset(); } } own{c};   // closed on every path
    rc = ensure_all(c->d_links_table, 2 * T.cap + LINKS_LIFTED_EXTRAS, c->d_links_recs, 2 * most, c->d_links_lift, 21 * n_scaf,
                    c->d_links_seq_size, n_seq);
    if (rc) { links_abandon(c); return rc; }
    T.keys = c->d_links_table; T.counts = T.keys + T.cap; T.extras = T.counts + T.cap;
    unsigned long long* rec_key = c->d_links_recs;
    unsigned long long* rec_cnt = rec_key + most;
    LiftTables d_lift;
    rc = lift_upload(c, c->d_links_lift, scaf_size, n_scaf, lift, &d_lift);
    if (!rc) rc = upload(c, c->d_links_seq_size, seq_size, sizeof(int64_t) * (size_t)n_seq);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(T.keys, 0xFF, sizeof(uint64_t) * (size_t)T.cap, c->stream));
    HIPCHK(hipMemsetAsync(T.counts, 0, sizeof(uint64_t) * (size_t)(T.cap + LINKS_LIFTED_EXTRAS), c->stream));
    if (c->pairs_len > 0) {
        launch_links_count_lifted(c->d_pairs_scaf_a, c->d_pairs_pos_a, c->d_pairs_scaf_b, c->d_pairs_pos_b, c->pairs_len, d_lift,
                                  c->d_links_seq_size, window, T, links_plain(), c->stream);
        HIPCHK(hipGetLastError());
        launch_links_compact(T, rec_key, rec_cnt, most, c->stream);
        HIPCHK(hipGetLastError());
    }
    uint64_t extras[LINKS_LIFTED_EXTRAS];
    rc = download(c, extras, T.extras, sizeof(extras));           // synchronises: the tables have left the upload arena
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
    for (int k = 0; k < LINKS_LIFTED_COUNTERS; k++) counters4_out[k] = extras[links_lifted_extra(k)];
    return HICMI_OK;
}
