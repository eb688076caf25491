// loader.hip - host-side HiC-Pro triplet parser (no device code): the "next" row N1 of SURVEY.md 8f.
//
// Replaces buildAdjacencyMatrix's line loop (scaffoldToChromosomes.py:70-98, orderGenome.py:65-93):
//   id1 <TAB> id2 <TAB> value  ->  dense fp64 matrix, each triplet mirrored, unknown bin IDs skipped,
//   a cell named twice keeps the value of the LATER line.
// The reference fills a Python list of lists (about 32 bytes per cell, minutes of interpreter time at
// N >= 16k).  Here the file is mmap'ed, cut into per-thread chunks at line boundaries and parsed with
// a correctly rounded decimal-to-double conversion (like Python's float()): Clinger's exact fast path
// for <= 15 significant digits - HiC-Pro prints 6 decimals - and glibc's strtod_l otherwise.  To keep "later line wins" exact under
// parallelism, parsed triplets are bucketed by the row block that owns the destination cell and each
// block is written by one thread walking the buckets in file order.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <charconv>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <clocale>
#include <cstdlib>
#include <locale.h>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>   // split.h's functions are __host__ __device__ under hipcc

#include "../../include/hicmi.h"
#include "split.h"

namespace hicmi { int set_error(int code, const char* msg); }   // api.hip: records the message for hicmi_last_error()

namespace {
struct Cell { int32_t r, c; double v; };

struct ParseError { bool bad = false; int64_t offset = 0; };

const double kPow10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16,
                           1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// Correctly rounded double from the decimal text [p, end).  Fast path (W. Clinger, 1990): with at most
// 15 significant digits the integer significand and 10^|e| (|e| <= 22) are both exact doubles, so one
// multiplication or division rounds once - the correctly rounded result.  Anything else (long
// significands, big exponents, inf/nan) goes to strtod_l in the "C" locale.
inline bool parse_double(const char* p, const char* end, const char* file_end, locale_t cloc, double& out)
{
    const char* q = p;
    bool neg = false;
    if (q < end && (*q == '-' || *q == '+')) { neg = *q == '-'; q++; }
    uint64_t w = 0; int digits = 0, dec_exp = 0; bool any = false, fast = true;
    while (q < end && *q >= '0' && *q <= '9') { any = true; if (w || *q != '0') { if (digits < 19) { w = w * 10 + (uint64_t)(*q - '0'); digits++; } else fast = false; } q++; }
    if (q < end && *q == '.') {
        q++;
        while (q < end && *q >= '0' && *q <= '9') {
            any = true;
            if (w || *q != '0') { if (digits < 19) { w = w * 10 + (uint64_t)(*q - '0'); digits++; dec_exp--; } else fast = false; }
            else dec_exp--;
            q++;
        }
    }
    if (any && q < end && (*q == 'e' || *q == 'E')) {
        const char* r = q + 1;
        bool eneg = false;
        if (r < end && (*r == '-' || *r == '+')) { eneg = *r == '-'; r++; }
        if (r < end && *r >= '0' && *r <= '9') {
            int ev = 0;
            while (r < end && *r >= '0' && *r <= '9') { if (ev < 10000) ev = ev * 10 + (*r - '0'); r++; }
            dec_exp += eneg ? -ev : ev;
            q = r;
        }
    }
    if (any && q == end && fast && digits <= 15 && dec_exp >= -22 && dec_exp <= 22) {
        double v = (double)w;
        v = dec_exp < 0 ? v / kPow10[-dec_exp] : v * kPow10[dec_exp];
        out = neg ? -v : v;
        return true;
    }
    // general case: strtod_l needs a terminator after the token; '\t', '\r', '\n' do that inside the
    // mapping, only a token that touches the end of the file is copied out
    char buf[512];
    const char* src = p;
    if (end == file_end) {
        size_t len = (size_t)(end - p);
        if (len >= sizeof(buf)) return false;
        memcpy(buf, p, len); buf[len] = 0;
        src = buf;
    }
    char* stop = nullptr;
    double v = strtod_l(src, &stop, cloc);
    if (stop != src + (end - p) || stop == src) return false;
    if (end - p > 1 && (src[0] == '0' || ((src[0] == '-' || src[0] == '+') && src[1] == '0')) &&
        (src[1] == 'x' || src[1] == 'X' || src[2] == 'x' || src[2] == 'X')) return false;     // float() has no hex form
    out = v;
    return true;
}

inline const char* parse_i64(const char* p, const char* end, int64_t& out, bool& ok)
{
    bool neg = false;
    if (p < end && (*p == '-' || *p == '+')) { neg = *p == '-'; p++; }
    if (p >= end || *p < '0' || *p > '9') { ok = false; return p; }
    int64_t v = 0;
    while (p < end && *p >= '0' && *p <= '9') { v = v * 10 + (*p - '0'); p++; }
    out = neg ? -v : v;
    return p;
}
}  // namespace

extern "C" int hicmi_load_hicpro_matrix(const char* path, const int64_t* bin_ids, int64_t n, double* out, int threads,
                                        int64_t* edges_out)
{
    auto hicmi_set_error = [](int code, const char* msg) { return hicmi::set_error(code, msg); };
    if (!path || !bin_ids || !out || n < 0) return hicmi_set_error(HICMI_EINVAL, "bad arguments");
    if (edges_out) *edges_out = 0;
    const bool prof = getenv("HICMI_LOADER_PROFILE") != nullptr;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    auto t_start = now();
    auto t_zero = now();
    int fd = open(path, O_RDONLY);
    if (fd < 0) return hicmi_set_error(HICMI_EINVAL, (std::string("cannot open ") + path).c_str());
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return hicmi_set_error(HICMI_EINVAL, "fstat failed"); }
    const size_t size = (size_t)st.st_size;
    if (size == 0 || n == 0) { close(fd); std::memset(out, 0, sizeof(double) * (size_t)n * (size_t)n); return HICMI_OK; }
    const char* data = (const char*)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (data == MAP_FAILED) return hicmi_set_error(HICMI_ENOMEM, "mmap failed");
    madvise((void*)data, size, MADV_SEQUENTIAL);

    int64_t max_id = -1;
    for (int64_t i = 0; i < n; i++) {
        if (bin_ids[i] < 0) { munmap((void*)data, size); return hicmi_set_error(HICMI_EINVAL, "negative bin ID"); }
        max_id = std::max(max_id, bin_ids[i]);
    }
    std::vector<int32_t> lookup((size_t)max_id + 2, -1);
    for (int64_t i = 0; i < n; i++) lookup[(size_t)bin_ids[i]] = (int32_t)i;      // a repeated ID keeps its last row, like a dict

    int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    T = std::max(1, std::min(T, 64));
    if (size < (size_t)T * 4096) T = 1;
    // chunk boundaries at line starts
    std::vector<size_t> cut((size_t)T + 1, size);
    cut[0] = 0;
    for (int t = 1; t < T; t++) {
        size_t p = size / (size_t)T * (size_t)t;
        while (p < size && data[p] != '\n') p++;
        cut[(size_t)t] = p < size ? p + 1 : size;
    }
    const int64_t rows_per = (n + T - 1) / T;
    std::vector<std::vector<std::vector<Cell>>> bucket((size_t)T, std::vector<std::vector<Cell>>((size_t)T));
    std::vector<ParseError> errs((size_t)T);
    std::vector<int64_t> edges((size_t)T, 0);

    locale_t cloc = newlocale(LC_ALL_MASK, "C", (locale_t)0);
    auto parse = [&](int t) {
        const char* p = data + cut[(size_t)t];
        const char* end = data + cut[(size_t)t + 1];
        auto& mine = bucket[(size_t)t];
        for (auto& b : mine) b.reserve((size_t)((end - p) / 24 / T + 16));
        while (p < end) {
            const char* eol = (const char*)memchr(p, '\n', (size_t)(end - p));
            if (!eol) eol = end;
            const char* le = eol;
            while (le > p && le[-1] == '\r') le--;                 // the reference strips '\r' and '\n' (S2C:82)
            if (le > p) {
                bool ok = true;
                int64_t a = 0, b = 0;
                const char* q = parse_i64(p, le, a, ok);
                if (ok && q < le && *q == '\t') q = parse_i64(q + 1, le, b, ok); else ok = false;
                double v = 0.0;
                if (ok && q < le && *q == '\t') {
                    q++;
                    while (q < le && (*q == ' ')) q++;             // float() tolerates surrounding blanks
                    const char* vend = (const char*)memchr(q, '\t', (size_t)(le - q));   // further columns are ignored (cols[2])
                    if (!vend) vend = le;
                    while (vend > q && vend[-1] == ' ') vend--;
                    if (q >= vend || !parse_double(q, vend, data + size, cloc, v)) ok = false;
                } else ok = false;
                if (!ok) { errs[(size_t)t].bad = true; errs[(size_t)t].offset = (int64_t)(p - data); return; }
                if (a >= 0 && a <= max_id && b >= 0 && b <= max_id) {
                    const int32_t ia = lookup[(size_t)a], ib = lookup[(size_t)b];
                    if (ia >= 0 && ib >= 0) {
                        mine[(size_t)(ia / rows_per)].push_back({ia, ib, v});
                        mine[(size_t)(ib / rows_per)].push_back({ib, ia, v});
                        edges[(size_t)t]++;
                    }
                }
            } else {
                // an empty line makes the reference raise (int('') at S2C:83); refuse it as well
                errs[(size_t)t].bad = true; errs[(size_t)t].offset = (int64_t)(p - data); return;
            }
            p = eol + 1;
        }
    };
    {
        std::vector<std::thread> pool;
        for (int t = 0; t < T; t++) pool.emplace_back(parse, t);
        for (auto& th : pool) th.join();
    }
    auto t_parse = now();
    if (cloc) freelocale(cloc);
    for (int t = 0; t < T; t++)
        if (errs[(size_t)t].bad) {
            munmap((void*)data, size);
            return hicmi_set_error(HICMI_EINVAL, (std::string("malformed triplet line at byte ") + std::to_string(errs[(size_t)t].offset)).c_str());
        }
    auto apply = [&](int owner) {
        // each owner zero-fills its own row block first: the page faults of the n*n output run in parallel
        const int64_t r0 = std::min<int64_t>(n, (int64_t)owner * rows_per), r1 = std::min<int64_t>(n, r0 + rows_per);
        if (r1 > r0) std::memset(out + (size_t)r0 * (size_t)n, 0, sizeof(double) * (size_t)(r1 - r0) * (size_t)n);
        for (int src = 0; src < T; src++)                          // file order: chunk by chunk, line by line
            for (const Cell& c : bucket[(size_t)src][(size_t)owner]) out[(size_t)c.r * (size_t)n + (size_t)c.c] = c.v;
    };
    {
        std::vector<std::thread> pool;
        for (int t = 0; t < T; t++) pool.emplace_back(apply, t);
        for (auto& th : pool) th.join();
    }
    auto t_apply = now();
    munmap((void*)data, size);
    if (prof) fprintf(stderr, "[hicmi] loader: %d threads, zero %.0f ms, parse %.0f ms, apply %.0f ms\n", T, ms(t_start, t_zero),
                      ms(t_zero, t_parse), ms(t_parse, t_apply));
    int64_t total = 0;
    for (int t = 0; t < T; t++) total += edges[(size_t)t];
    if (edges_out) *edges_out = total;
    return HICMI_OK;
}

// ---- valid-pair scan (orientSmallScaffolds.py:159-177 readValidPairFile) ---------
// HiC-Pro allValidPairs lines: read <TAB> scaffold1 <TAB> pos1 <TAB> strand1 <TAB> scaffold2 <TAB> pos2 ...
// The reference keeps, for every ORDERED pair of neighbouring scaffold names it registered, the two positions of
// each line naming that pair; everything else in a multi-GB file is skipped.  Same host-side scheme as the
// matrix loader: mmap, per-thread chunks cut at line starts, hits collected per thread and concatenated in
// thread order = file order.
#include <unordered_map>
#include <string_view>

namespace {
struct PairHit { int32_t pair; int64_t p1, p2; };
struct ScanResult { std::vector<PairHit> hits; };

inline bool parse_pos(const char* p, const char* end, int64_t& out)
{
    // Python int(): optional sign, digits, surrounding blanks tolerated
    while (p < end && (*p == ' ')) p++;
    while (end > p && (end[-1] == ' ')) end--;
    bool ok = true;
    const char* q = parse_i64(p, end, out, ok);
    return ok && q == end;
}

using NameMap = std::unordered_map<std::string_view, int32_t>;

// names_blob / name_off[n_names + 1] -> index of every name (a name given twice keeps its first index)
NameMap make_name_map(const char* names_blob, const int64_t* name_off, int64_t n_names)
{
    NameMap name_id;
    name_id.reserve((size_t)n_names * 2);
    for (int64_t i = 0; i < n_names; i++)
        name_id.emplace(std::string_view(names_blob + name_off[i], (size_t)(name_off[i + 1] - name_off[i])), (int32_t)i);
    return name_id;
}

// the starts of the columns 0 .. 6 of the line [p, le): returns how many there are (7 = "seven or more"); column k ends
// at col[k + 1] - 1, the last one at le
inline int split_cols(const char* p, const char* le, const char* col[7])
{
    int nc = 0;
    col[nc++] = p;
    for (const char* q = p; nc < 7;) {
        const char* tab = (const char*)memchr(q, '\t', (size_t)(le - q));
        if (!tab) break;
        col[nc++] = tab + 1;
        q = tab + 1;
    }
    return nc;
}

// a read-only mapping of a whole file; size 0 maps nothing
struct MappedFile {
    const char* data = nullptr; size_t size = 0;
    ~MappedFile() { if (data) munmap((void*)data, size); }
    // HICMI_OK, or the code recorded with hicmi::set_error
    int open_path(const char* path)
    {
        int fd = open(path, O_RDONLY);
        if (fd < 0) return hicmi::set_error(HICMI_EINVAL, (std::string("cannot open ") + path).c_str());
        struct stat st;
        if (fstat(fd, &st) != 0) { close(fd); return hicmi::set_error(HICMI_EINVAL, "fstat failed"); }
        size = (size_t)st.st_size;
        if (size == 0) { close(fd); return HICMI_OK; }
        void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        close(fd);
        if (m == MAP_FAILED) { size = 0; return hicmi::set_error(HICMI_ENOMEM, "mmap failed"); }
        data = (const char*)m;
        madvise((void*)data, size, MADV_SEQUENTIAL);
        return HICMI_OK;
    }
};
}  // namespace

extern "C" int hicmi_scan_valid_pairs(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names,
                                      const int32_t* pair_a, const int32_t* pair_b, int64_t n_pairs, int threads,
                                      int64_t* n_hits_out, int64_t* n_lines_out, void** handle_out)
{
    auto err = [](int code, const std::string& msg) { return hicmi::set_error(code, msg.c_str()); };
    if (!path || !names_blob || !name_off || !n_hits_out || !n_lines_out || !handle_out || n_names < 0 || n_pairs < 0 ||
        (n_pairs > 0 && (!pair_a || !pair_b)))
        return err(HICMI_EINVAL, "bad arguments");
    *n_hits_out = 0; *n_lines_out = 0; *handle_out = nullptr;
    const NameMap name_id = make_name_map(names_blob, name_off, n_names);
    std::unordered_map<uint64_t, int32_t> pair_id;
    pair_id.reserve((size_t)n_pairs * 2);
    for (int64_t i = 0; i < n_pairs; i++) {
        if (pair_a[i] < 0 || pair_a[i] >= n_names || pair_b[i] < 0 || pair_b[i] >= n_names) return err(HICMI_EINVAL, "pair names out of range");
        pair_id[((uint64_t)(uint32_t)pair_a[i] << 32) | (uint32_t)pair_b[i]] = (int32_t)i;
    }
    int fd = open(path, O_RDONLY);
    if (fd < 0) return err(HICMI_EINVAL, std::string("cannot open ") + path);
    struct stat st;
    if (fstat(fd, &st) != 0) { close(fd); return err(HICMI_EINVAL, "fstat failed"); }
    const size_t size = (size_t)st.st_size;
    auto* res = new ScanResult();
    if (size == 0) { close(fd); *handle_out = res; return HICMI_OK; }
    const char* data = (const char*)mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (data == MAP_FAILED) { delete res; return err(HICMI_ENOMEM, "mmap failed"); }
    madvise((void*)data, size, MADV_SEQUENTIAL);
    int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    T = std::max(1, std::min(T, 64));
    if (size < (size_t)T * 4096) T = 1;
    std::vector<size_t> cut((size_t)T + 1, size);
    cut[0] = 0;
    for (int t = 1; t < T; t++) {
        size_t p = size / (size_t)T * (size_t)t;
        while (p < size && data[p] != '\n') p++;
        cut[(size_t)t] = p < size ? p + 1 : size;
    }
    std::vector<std::vector<PairHit>> part((size_t)T);
    std::vector<int64_t> lines((size_t)T, 0), bad((size_t)T, -1);
    auto work = [&](int t) {
        const char* p = data + cut[(size_t)t];
        const char* end = data + cut[(size_t)t + 1];
        auto& out = part[(size_t)t];
        while (p < end) {
            const char* eol = (const char*)memchr(p, '\n', (size_t)(end - p));
            if (!eol) eol = end;
            const char* le = eol;
            while (le > p && le[-1] == '\r') le--;
            // columns 0..5
            const char* col[7];
            const int nc = split_cols(p, le, col);
            // the reference indexes cols[1] and cols[4] on every line (orientSmallScaffolds.py:168) and cols[2], cols[5]
            // only for a registered pair (:170): a 5-column line that names no such pair is accepted there, so it is here
            if (nc < 5) { bad[(size_t)t] = (int64_t)(p - data); return; }   // cols[4] missing: IndexError in the reference
            const char* c4_end = nc >= 6 ? col[5] - 1 : le;
            const char* c5_end = nc >= 7 ? col[6] - 1 : le;
            lines[(size_t)t]++;
            auto a = name_id.find(std::string_view(col[1], (size_t)(col[2] - 1 - col[1])));
            if (a != name_id.end()) {
                auto b = name_id.find(std::string_view(col[4], (size_t)(c4_end - col[4])));
                if (b != name_id.end()) {
                    auto hit = pair_id.find(((uint64_t)(uint32_t)a->second << 32) | (uint32_t)b->second);
                    if (hit != pair_id.end()) {
                        if (nc < 6) { bad[(size_t)t] = (int64_t)(p - data); return; }   // cols[5] missing on a hit: IndexError there too
                        int64_t p1 = 0, p2 = 0;
                        if (!parse_pos(col[2], col[3] - 1, p1) || !parse_pos(col[5], c5_end, p2)) { bad[(size_t)t] = (int64_t)(p - data); return; }
                        out.push_back({hit->second, p1, p2});
                    }
                }
            }
            p = eol + 1;
        }
    };
    {
        std::vector<std::thread> pool;
        for (int t = 0; t < T; t++) pool.emplace_back(work, t);
        for (auto& th : pool) th.join();
    }
    munmap((void*)data, size);
    for (int t = 0; t < T; t++)
        if (bad[(size_t)t] >= 0) { delete res; return err(HICMI_EINVAL, "malformed valid-pair line at byte " + std::to_string(bad[(size_t)t])); }
    size_t total = 0;
    for (auto& v : part) total += v.size();
    res->hits.reserve(total);
    for (auto& v : part) res->hits.insert(res->hits.end(), v.begin(), v.end());
    int64_t n_lines = 0;
    for (auto v : lines) n_lines += v;
    *n_hits_out = (int64_t)total; *n_lines_out = n_lines; *handle_out = res;
    return HICMI_OK;
}

extern "C" int hicmi_scan_fetch(void* handle, int32_t* pair_idx, int64_t* pos1, int64_t* pos2)
{
    if (!handle) return hicmi::set_error(HICMI_EINVAL, "NULL handle");
    auto* res = reinterpret_cast<ScanResult*>(handle);
    if (!res->hits.empty() && (!pair_idx || !pos1 || !pos2)) return hicmi::set_error(HICMI_EINVAL, "NULL output");
    for (size_t i = 0; i < res->hits.size(); i++) { pair_idx[i] = res->hits[i].pair; pos1[i] = res->hits[i].p1; pos2[i] = res->hits[i].p2; }
    delete res;
    return HICMI_OK;
}

// ---- chunked valid-pair parser (buildMap) -------------------------------------------------------------------
// The scan above keeps the few lines of registered pairs; this one keeps every line whose two ends lie on known
// scaffolds, `max_pairs` at a time, for the device to count.  A window of bytes sized for the pairs still wanted is cut at
// line starts into one part per thread; the parts are taken in file order, and the part in which the quota is reached is
// parsed again by one thread that stops right after the line of the last pair wanted.  So the pairs, the statistics and
// next_byte of a call depend on the file and on max_pairs alone, never on the number of threads.
namespace {
struct PairRec { int32_t sa, sb; int64_t pa, pb; };
struct PairPart { std::vector<PairRec> recs; int64_t lines = 0, unknown = 0, out_of_range = 0, bad = -1; };

// Parses the whole lines of [begin, end) until `quota` pairs are kept; returns where it stopped (a line start, or end).
// A malformed line sets part.bad to its offset and stops there.
const char* parse_pair_lines(const char* data, const char* begin, const char* end, int64_t quota, const NameMap& name_id,
                             const int64_t* scaf_size, PairPart& part)
{
    const char* p = begin;
    std::string_view last_name[2];                     // the file is sorted by scaffold: the previous line's names first
    int32_t last_id[2] = {-1, -1};
    auto lookup = [&](int k, const char* s, const char* e) -> int32_t {
        const std::string_view name(s, (size_t)(e - s));
        if (last_name[k].data() && name == last_name[k]) return last_id[k];
        const auto it = name_id.find(name);
        last_name[k] = name;
        return last_id[k] = it == name_id.end() ? -1 : it->second;
    };
    while (p < end && (int64_t)part.recs.size() < quota) {
        const char* eol = (const char*)memchr(p, '\n', (size_t)(end - p));
        if (!eol) eol = end;
        const char* le = eol;
        while (le > p && le[-1] == '\r') le--;
        const char* col[7];
        const int nc = split_cols(p, le, col);
        int64_t p1 = 0, p2 = 0;
        if (nc < 6 || !parse_pos(col[2], col[3] - 1, p1) || !parse_pos(col[5], nc >= 7 ? col[6] - 1 : le, p2)) {
            part.bad = (int64_t)(p - data);
            return p;
        }
        part.lines++;
        const int32_t a = lookup(0, col[1], col[2] - 1), b = lookup(1, col[4], col[5] - 1);
        if (a < 0 || b < 0) part.unknown++;
        else if (p1 < 1 || p1 > scaf_size[a] || p2 < 1 || p2 > scaf_size[b]) part.out_of_range++;
        else part.recs.push_back({a, b, p1, p2});
        p = eol < end ? eol + 1 : end;
    }
    return p;
}
}  // namespace

extern "C" int hicmi_parse_valid_pairs(const char* path, const char* names_blob, const int64_t* name_off, int64_t n_names,
                                       const int64_t* scaf_size, int threads, int64_t first_byte, int64_t max_pairs,
                                       int32_t* scaf_a, int64_t* pos_a, int32_t* scaf_b, int64_t* pos_b, int64_t* n_out,
                                       int64_t* next_byte_out, int64_t* stats4)
{
    auto err = [](int code, const std::string& msg) { return hicmi::set_error(code, msg.c_str()); };
    if (!path || !names_blob || !name_off || !n_out || !next_byte_out || !stats4 || n_names < 0 || (n_names > 0 && !scaf_size) ||
        first_byte < 0 || max_pairs < 1 || !scaf_a || !pos_a || !scaf_b || !pos_b)
        return err(HICMI_EINVAL, "bad arguments");
    *n_out = 0; *next_byte_out = first_byte;
    for (int k = 0; k < 4; k++) stats4[k] = 0;
    const NameMap name_id = make_name_map(names_blob, name_off, n_names);
    MappedFile file;
    if (int rc = file.open_path(path)) return rc;
    const size_t size = file.size;
    const char* data = file.data;
    if ((uint64_t)first_byte > size) return err(HICMI_EINVAL, "first_byte " + std::to_string(first_byte) + " is beyond the end of the file");
    int T_max = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    T_max = std::max(1, std::min(T_max, 64));
    int64_t kept = 0, lines = 0, unknown = 0, out_of_range = 0;
    auto emit = [&](const PairPart& part) {
        for (const PairRec& r : part.recs) { scaf_a[kept] = r.sa; pos_a[kept] = r.pa; scaf_b[kept] = r.sb; pos_b[kept] = r.pb; kept++; }
        lines += part.lines; unknown += part.unknown; out_of_range += part.out_of_range;
    };
    auto malformed = [&](int64_t off) { return err(HICMI_EINVAL, "malformed valid-pair line at byte " + std::to_string(off)); };
    size_t pos = (size_t)first_byte;
    while (pos < size && kept < max_pairs) {
        // a window for the pairs still wanted (a full 12-column line is about 60 bytes), closed at a line end
        const int64_t want = max_pairs - kept;
        size_t w_end = size;
        if ((uint64_t)want < (size - pos) / 64) {
            w_end = std::min(size, pos + std::max<size_t>((size_t)want * 64, (size_t)1 << 12));
            const char* nl = w_end < size ? (const char*)memchr(data + w_end, '\n', size - w_end) : nullptr;
            w_end = nl ? (size_t)(nl - data) + 1 : size;
        }
        const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)T_max, (w_end - pos) / 4096));
        std::vector<size_t> cut((size_t)T + 1, w_end);
        cut[0] = pos;
        for (int t = 1; t < T; t++) {
            size_t p = pos + (w_end - pos) / (size_t)T * (size_t)t;
            while (p < w_end && data[p] != '\n') p++;
            cut[(size_t)t] = p < w_end ? p + 1 : w_end;
        }
        std::vector<PairPart> part((size_t)T);
        auto work = [&](int t) {
            part[(size_t)t].recs.reserve((cut[(size_t)t + 1] - cut[(size_t)t]) / 40 + 16);
            parse_pair_lines(data, data + cut[(size_t)t], data + cut[(size_t)t + 1], INT64_MAX, name_id, scaf_size, part[(size_t)t]);
        };
        {
            std::vector<std::thread> pool;
            for (int t = 1; t < T; t++) pool.emplace_back(work, t);
            work(0);
            for (auto& th : pool) th.join();
        }
        for (int t = 0; t < T && kept < max_pairs; t++) {
            const PairPart& mine = part[(size_t)t];
            if (kept + (int64_t)mine.recs.size() < max_pairs) {
                if (mine.bad >= 0) return malformed(mine.bad);
                emit(mine);
                pos = cut[(size_t)t + 1];
            } else {
                // the quota is reached inside this part: once more, stopping right after the line of the last pair wanted
                PairPart again;
                again.recs.reserve((size_t)(max_pairs - kept));
                const char* stop = parse_pair_lines(data, data + cut[(size_t)t], data + cut[(size_t)t + 1], max_pairs - kept, name_id,
                                                    scaf_size, again);
                if (again.bad >= 0) return malformed(again.bad);
                emit(again);
                pos = (size_t)(stop - data);
            }
        }
    }
    *n_out = kept; *next_byte_out = (int64_t)pos;
    stats4[0] = lines; stats4[1] = kept; stats4[2] = unknown; stats4[3] = out_of_range;
    return HICMI_OK;
}

// ---- valid pairs rewritten onto the pieces of cut scaffolds (splitScaffolds) ------------------------------------
// Every line the chunked parser keeps is written again with its columns 1, 2, 4 and 5 - scaffold and position of both
// ends - replaced by the piece and the position in the piece (split.h); every other byte of the line stays.  The lines
// the parser skips are dropped.  A window of the file is cut at line starts into one part per thread, and the parts are
// written in file order: a line is rewritten on its own, so the bytes written do not depend on the number of threads.
namespace {
struct SplitPart { std::string text; int64_t lines = 0, kept = 0, unknown = 0, out_of_range = 0, bad = -1; };

void rewrite_pair_lines(const char* data, const char* begin, const char* end, const NameMap& name_id, const int64_t* scaf_size,
                        const hicmi::SplitTables& tables, const char* piece_names, const int64_t* piece_name_off, SplitPart& part)
{
    const char* p = begin;
    std::string_view last_name[2];                     // as in parse_pair_lines: the previous line's names first
    int32_t last_id[2] = {-1, -1};
    auto lookup = [&](int k, const char* s, const char* e) -> int32_t {
        const std::string_view name(s, (size_t)(e - s));
        if (last_name[k].data() && name == last_name[k]) return last_id[k];
        const auto it = name_id.find(name);
        last_name[k] = name;
        return last_id[k] = it == name_id.end() ? -1 : it->second;
    };
    auto put_end = [&](int32_t piece, int64_t pos) {
        part.text.append(piece_names + piece_name_off[piece], (size_t)(piece_name_off[piece + 1] - piece_name_off[piece]));
        part.text.push_back('\t');
        char digits[24];
        const auto r = std::to_chars(digits, digits + sizeof(digits), (long long)pos);
        part.text.append(digits, (size_t)(r.ptr - digits));
    };
    while (p < end) {
        const char* eol = (const char*)memchr(p, '\n', (size_t)(end - p));
        if (!eol) eol = end;
        const char* le = eol;
        while (le > p && le[-1] == '\r') le--;
        const char* col[7];
        const int nc = split_cols(p, le, col);
        const char* c5_end = nc >= 7 ? col[6] - 1 : le;
        int64_t p1 = 0, p2 = 0;
        if (nc < 6 || !parse_pos(col[2], col[3] - 1, p1) || !parse_pos(col[5], c5_end, p2)) {
            part.bad = (int64_t)(p - data);
            return;
        }
        part.lines++;
        const char* next = eol < end ? eol + 1 : end;
        const int32_t a = lookup(0, col[1], col[2] - 1), b = lookup(1, col[4], col[5] - 1);
        if (a < 0 || b < 0) part.unknown++;
        else if (p1 < 1 || p1 > scaf_size[a] || p2 < 1 || p2 > scaf_size[b]) part.out_of_range++;
        else {
            int64_t x1, x2;
            const int32_t k1 = hicmi::split_end(tables, a, p1, &x1), k2 = hicmi::split_end(tables, b, p2, &x2);
            part.text.append(p, (size_t)(col[1] - p));                         // column 0 and its tab
            put_end(k1, x1);
            part.text.append(col[3] - 1, (size_t)(col[4] - (col[3] - 1)));     // the tab, column 3 and its tab
            put_end(k2, x2);
            part.text.append(c5_end, (size_t)(next - c5_end));                 // the further columns and the line end as they are
            part.kept++;
        }
        p = next;
    }
}
}  // namespace

extern "C" int hicmi_split_valid_pairs(const char* path_in, const char* path_out, const char* names_blob, const int64_t* name_off,
                                       int64_t n_names, const int64_t* scaf_size, const int32_t* piece_first, const int64_t* piece_start,
                                       int64_t n_piece, const char* piece_names_blob, const int64_t* piece_name_off, int threads,
                                       int64_t* stats4)
{
    auto err = [](int code, const std::string& msg) { return hicmi::set_error(code, msg.c_str()); };
    if (!path_in || !path_out || !names_blob || !name_off || !scaf_size || !piece_first || !piece_start || !piece_names_blob ||
        !piece_name_off || !stats4 || n_names < 1 || n_names > INT32_MAX / 4 || n_piece < n_names || n_piece > INT32_MAX / 4)
        return err(HICMI_EINVAL, "bad arguments");
    for (int k = 0; k < 4; k++) stats4[k] = 0;
    char msg[256];
    if (hicmi::split_check_tables(scaf_size, n_names, piece_first, piece_start, n_piece, msg, sizeof(msg))) return err(HICMI_EINVAL, msg);
    hicmi::SplitTables tables;
    tables.piece_first = piece_first; tables.piece_start = piece_start;
    tables.n_scaf = (int32_t)n_names; tables.n_piece = (int32_t)n_piece;
    const NameMap name_id = make_name_map(names_blob, name_off, n_names);
    MappedFile file;
    if (int rc = file.open_path(path_in)) return rc;
    const size_t size = file.size;
    const char* data = file.data;
    // written under a temporary name and renamed when it is whole: an error leaves no output file behind
    const std::string tmp = std::string(path_out) + ".part";
    FILE* fh = fopen(tmp.c_str(), "wb");
    if (!fh) return err(HICMI_EINVAL, std::string("cannot open ") + tmp + " for writing");
    auto give_up = [&](int code, const std::string& what) { fclose(fh); remove(tmp.c_str()); return err(code, what); };
    int T_max = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    T_max = std::max(1, std::min(T_max, 64));
    constexpr size_t kWindow = (size_t)64 << 20;
    int64_t lines = 0, kept = 0, unknown = 0, out_of_range = 0;
    size_t pos = 0;
    while (pos < size) {
        size_t w_end = size;
        if (size - pos > kWindow) {
            const char* nl = (const char*)memchr(data + pos + kWindow, '\n', size - pos - kWindow);
            w_end = nl ? (size_t)(nl - data) + 1 : size;
        }
        const int T = (int)std::max<size_t>(1, std::min<size_t>((size_t)T_max, (w_end - pos) / 4096));
        std::vector<size_t> cut((size_t)T + 1, w_end);
        cut[0] = pos;
        for (int t = 1; t < T; t++) {
            size_t p = pos + (w_end - pos) / (size_t)T * (size_t)t;
            while (p < w_end && data[p] != '\n') p++;
            cut[(size_t)t] = p < w_end ? p + 1 : w_end;
        }
        std::vector<SplitPart> part((size_t)T);
        auto work = [&](int t) {
            part[(size_t)t].text.reserve(cut[(size_t)t + 1] - cut[(size_t)t] + 64);
            rewrite_pair_lines(data, data + cut[(size_t)t], data + cut[(size_t)t + 1], name_id, scaf_size, tables, piece_names_blob,
                               piece_name_off, part[(size_t)t]);
        };
        {
            std::vector<std::thread> pool;
            for (int t = 1; t < T; t++) pool.emplace_back(work, t);
            work(0);
            for (auto& th : pool) th.join();
        }
        for (const SplitPart& mine : part) {
            // the parts are in file order and each stops at its first malformed line: this is the first one of the file
            if (mine.bad >= 0) return give_up(HICMI_EINVAL, "malformed valid-pair line at byte " + std::to_string(mine.bad));
            if (!mine.text.empty() && fwrite(mine.text.data(), 1, mine.text.size(), fh) != mine.text.size())
                return give_up(HICMI_EINVAL, std::string("write error on ") + tmp);
            lines += mine.lines; kept += mine.kept; unknown += mine.unknown; out_of_range += mine.out_of_range;
        }
        pos = w_end;
    }
    if (fclose(fh) != 0) { remove(tmp.c_str()); return err(HICMI_EINVAL, std::string("write error on ") + tmp); }
    if (rename(tmp.c_str(), path_out) != 0) { remove(tmp.c_str()); return err(HICMI_EINVAL, std::string("cannot rename ") + tmp + " to " + path_out); }
    stats4[0] = lines; stats4[1] = kept; stats4[2] = unknown; stats4[3] = out_of_range;
    return HICMI_OK;
}

// ---- writer of HiC-Pro's *_iced.matrix (-part0) -------------------------------------------------------------------------
namespace {
// Python's repr(float): the shortest digits that read back to the same double (std::to_chars), laid out by CPython's
// rule - fixed notation while the decimal point falls in (-4, 16], else d.ddde+XX with at least two exponent digits
char* put_repr(char* p, double v)
{
    if (std::isnan(v)) { memcpy(p, "nan", 3); return p + 3; }
    if (std::isinf(v)) { if (v < 0) *p++ = '-'; memcpy(p, "inf", 3); return p + 3; }
    char buf[48];
    const auto r = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::scientific);
    const char* s = buf;
    if (*s == '-') *p++ = *s++;
    const char* e = s;
    while (e < r.ptr && *e != 'e') e++;
    char dig[24];
    int nd = 0;
    dig[nd++] = s[0];
    if (s + 1 < e && s[1] == '.')
        for (const char* q = s + 2; q < e; q++) dig[nd++] = *q;
    int ex = 0;
    {
        const char* q = e + 1;
        const bool neg = q < r.ptr && *q == '-';
        if (q < r.ptr && (*q == '-' || *q == '+')) q++;
        for (; q < r.ptr; q++) ex = ex * 10 + (*q - '0');
        if (neg) ex = -ex;
    }
    const int decpt = ex + 1;
    if (-4 < decpt && decpt <= 16) {
        if (decpt <= 0) {
            *p++ = '0'; *p++ = '.';
            for (int k = 0; k < -decpt; k++) *p++ = '0';
            memcpy(p, dig, (size_t)nd); p += nd;
        } else if (decpt >= nd) {
            memcpy(p, dig, (size_t)nd); p += nd;
            for (int k = nd; k < decpt; k++) *p++ = '0';
            *p++ = '.'; *p++ = '0';
        } else {
            memcpy(p, dig, (size_t)decpt); p += decpt;
            *p++ = '.';
            memcpy(p, dig + decpt, (size_t)(nd - decpt)); p += nd - decpt;
        }
    } else {
        *p++ = dig[0];
        if (nd > 1) { *p++ = '.'; memcpy(p, dig + 1, (size_t)(nd - 1)); p += nd - 1; }
        *p++ = 'e';
        *p++ = ex < 0 ? '-' : '+';
        const int a = ex < 0 ? -ex : ex;
        if (a >= 100) *p++ = (char)('0' + a / 100);
        *p++ = (char)('0' + a / 10 % 10);
        *p++ = (char)('0' + a % 10);
    }
    return p;
}
}  // namespace

extern "C" int hicmi_format_double(double v, char* out, int64_t cap)
{
    char buf[64];
    const int64_t len = put_repr(buf, v) - buf;
    if (!out || cap < len + 1) return hicmi::set_error(HICMI_EINVAL, "output buffer too small");
    memcpy(out, buf, (size_t)len);
    out[len] = 0;
    return HICMI_OK;
}

extern "C" int hicmi_write_hicpro_matrix(const char* path, const double* mat, int64_t n, const int64_t* bin_ids, int threads,
                                         int64_t* entries_out)
{
    if (!path || !mat || !bin_ids || n < 0) return hicmi::set_error(HICMI_EINVAL, "bad arguments");
    std::vector<std::string> ids((size_t)n);
    for (int64_t i = 0; i < n; i++) ids[(size_t)i] = std::to_string((long long)bin_ids[i]);
    FILE* fh = fopen(path, "wb");
    if (!fh) return hicmi::set_error(HICMI_EINVAL, (std::string("cannot open ") + path + " for writing").c_str());
    int T = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    T = std::max(1, std::min(T, 64));
    constexpr int64_t kRows = 16;                           // rows per work item
    const int64_t n_items = (n + kRows - 1) / kRows, per_round = (int64_t)T * 4;
    std::vector<std::string> text((size_t)per_round);
    std::vector<int64_t> count((size_t)per_round);
    int64_t entries = 0;
    bool io_error = false;
    for (int64_t base = 0; base < n_items && !io_error; base += per_round) {
        const int64_t here = std::min(per_round, n_items - base);
        std::atomic<int64_t> next{0};
        auto work = [&]() {
            for (;;) {
                const int64_t k = next.fetch_add(1);
                if (k >= here) return;
                std::string& t = text[(size_t)k];
                t.clear();
                int64_t cnt = 0;
                char line[128];
                const int64_t r0 = (base + k) * kRows, r1 = std::min(n, r0 + kRows);
                for (int64_t i = r0; i < r1; i++) {
                    const double* row = mat + i * n;
                    const std::string& a = ids[(size_t)i];
                    for (int64_t j = i; j < n; j++) {
                        if (row[j] == 0.0) continue;
                        char* p = line;
                        memcpy(p, a.data(), a.size()); p += a.size();
                        *p++ = '\t';
                        const std::string& b = ids[(size_t)j];
                        memcpy(p, b.data(), b.size()); p += b.size();
                        *p++ = '\t';
                        p = put_repr(p, row[j]);
                        *p++ = '\n';
                        t.append(line, (size_t)(p - line));
                        cnt++;
                    }
                }
                count[(size_t)k] = cnt;
            }
        };
        std::vector<std::thread> pool;
        for (int t = 1; t < T && t < here; t++) pool.emplace_back(work);
        work();
        for (auto& th : pool) th.join();
        for (int64_t k = 0; k < here; k++) {
            const std::string& t = text[(size_t)k];
            if (!t.empty() && fwrite(t.data(), 1, t.size(), fh) != t.size()) io_error = true;
            entries += count[(size_t)k];
        }
    }
    if (fclose(fh) != 0) io_error = true;
    if (io_error) return hicmi::set_error(HICMI_EINVAL, (std::string("write error on ") + path).c_str());
    if (entries_out) *entries_out = entries;
    return HICMI_OK;
}
