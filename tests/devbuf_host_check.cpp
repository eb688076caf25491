// devbuf_host_check.cpp - DevBuf, PinBuf and reserve_all of csrc/devbuf.h as host code, for a build with
// -fsanitize=address,undefined (tests/test_devbuf_cpu.py builds and runs it).  No HIP runtime is linked: the five calls
// the header makes are defined here over malloc, count their live blocks and can be told to fail their k-th allocation.
// Every block is a heap block of exactly its size, so the sanitizer sees a leak, a double free or a write past the end.
// Exit status 0 and "devbuf: OK" only if every check held and no block is alive at the end.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "devbuf.h"

using namespace hicmi;

static std::set<void*> g_live, g_live_pinned;
static long g_allocs = 0, g_frees = 0, g_fail_at = -1;   // g_fail_at: the allocation call (counted from 0) that fails
static size_t g_last_bytes = 0;
static int g_bad = 0;

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_bad++; }                 \
    } while (0)

static hipError_t stub_alloc(std::set<void*>& live, void** p, size_t bytes)
{
    if (g_allocs++ == g_fail_at) { *p = reinterpret_cast<void*>(0x10); return hipErrorOutOfMemory; }   // (a failed call's pointer is garbage)
    *p = malloc(bytes);
    g_last_bytes = bytes;
    live.insert(*p);
    return hipSuccess;
}

static hipError_t stub_free(std::set<void*>& live, void* p)
{
    g_frees++;
    if (!live.erase(p)) { printf("FAILED: free of a block that is not alive (double free?)\n"); g_bad++; return hipErrorInvalidValue; }
    free(p);
    return hipSuccess;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(g_live, p, bytes); }
hipError_t hipFree(void* p) { return stub_free(g_live, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return stub_alloc(g_live_pinned, p, bytes); }
hipError_t hipHostFree(void* p) { return stub_free(g_live_pinned, p); }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub error"; }
}

static void fail_call(long k) { g_fail_at = g_allocs + k; }   // the k-th allocation from now on fails

template <typename Buf>
static void check_one_buffer(std::set<void*>& live)
{
    const size_t elem = Buf::bytes_for(1);
    {
        Buf b;
        CHECK(b.get() == nullptr && b.capacity() == 0 && !b);
        CHECK(b.reserve(100) == hipSuccess && b.get() && b.capacity() == 100 && g_last_bytes == 100 * elem && live.size() == 1);
        b.get()[99] = {};                                          // the last element is inside the block
        auto* p = b.get();
        long frees = g_frees;
        CHECK(b.reserve(100) == hipSuccess && b.get() == p && b.capacity() == 100);      // equal: kept
        CHECK(b.reserve(7) == hipSuccess && b.get() == p && b.capacity() == 100);        // smaller: kept, never shrinks
        CHECK(b.reserve(0) == hipSuccess && b.get() == p && g_frees == frees);
        CHECK(b.reserve(101) == hipSuccess && b.capacity() == 101 && g_frees == frees + 1 && live.size() == 1);   // larger: one free, then one block
        CHECK(static_cast<decltype(p)>(b) == b.get());             // the implicit conversion kernels' arguments use
        // a failed reserve: empty, and nothing of this buffer alive
        fail_call(0);
        CHECK(b.reserve(1000) == hipErrorOutOfMemory && b.get() == nullptr && b.capacity() == 0 && live.empty());
        CHECK(b.reserve(5) == hipSuccess && b.capacity() == 5 && live.size() == 1);      // usable again
        b.reset();
        CHECK(b.get() == nullptr && b.capacity() == 0 && live.empty());
        b.reset();                                                 // (twice is harmless)
        // need <= 0: one element
        CHECK(b.reserve(0) == hipSuccess && b.capacity() == 1 && g_last_bytes == elem);
        b.reset();
        CHECK(b.reserve(-1) == hipSuccess && b.capacity() == 1 && g_last_bytes == elem && live.size() == 1);
        // moving empties the source
        Buf c(std::move(b));
        CHECK(b.get() == nullptr && b.capacity() == 0 && c.get() && c.capacity() == 1 && live.size() == 1);
        Buf d;
        CHECK(d.reserve(3) == hipSuccess && live.size() == 2);
        auto* pc = c.get();
        d = std::move(c);                                          // the target's old block is freed
        CHECK(c.get() == nullptr && c.capacity() == 0 && d.get() == pc && d.capacity() == 1 && live.size() == 1);
    }
    CHECK(live.empty());                                           // scope exit frees
}

static void check_group()
{
    const int64_t need[4] = {10, 20, 0, 40};                       // (0: one element)
    const size_t bytes[4] = {10 * sizeof(double), 20 * sizeof(int32_t), 1, 40 * sizeof(uint16_t)};
    DevBuf<double> a; DevBuf<int32_t> b; DevBuf<unsigned char> c; DevBuf<uint16_t> d;
    for (int round = 0; round < 2; round++)                        // from empty buffers, then from buffers that hold smaller blocks
        for (long k = 0; k < 4; k++) {
            if (round) CHECK(a.reserve(1) == hipSuccess && b.reserve(1) == hipSuccess && d.reserve(1) == hipSuccess && g_live.size() == 3);
            size_t failed = 0;
            fail_call(k);
            CHECK(reserve_all(&failed, a, need[0], b, need[1], c, need[2], d, need[3]) == hipErrorOutOfMemory);
            CHECK(failed == bytes[k]);
            CHECK(!a && !b && !c && !d && a.capacity() == 0 && b.capacity() == 0 && c.capacity() == 0 && d.capacity() == 0);
            CHECK(g_live.empty());
        }
    size_t failed = 0;
    g_fail_at = -1;
    CHECK(reserve_all(&failed, a, need[0], b, need[1], c, need[2], d, need[3]) == hipSuccess && failed == 0);
    CHECK(a && b && c && d && a.capacity() == 10 && b.capacity() == 20 && c.capacity() == 1 && d.capacity() == 40 && g_live.size() == 4);
    // a group that already holds enough is left alone, member by member
    double* pa = a; uint16_t* pd = d;
    const long allocs = g_allocs;
    CHECK(reserve_all(&failed, a, 10, b, 5, c, 1, d, 40) == hipSuccess && a.get() == pa && d.get() == pd && g_allocs == allocs);
    // one member grows and fails: the members that needed nothing are emptied too
    fail_call(0);
    CHECK(reserve_all(&failed, a, 10, b, 21, c, 1, d, 40) == hipErrorOutOfMemory && failed == 21 * sizeof(int32_t));
    CHECK(!a && !b && !c && !d && g_live.empty());
    // a pinned and a device buffer in one group
    PinBuf<char> p;
    CHECK(reserve_all(&failed, p, 64, a, 8) == hipSuccess && g_live.size() == 1 && g_live_pinned.size() == 1);
    fail_call(1);
    CHECK(reserve_all(&failed, p, 128, a, 16) == hipErrorOutOfMemory && !p && !a && g_live.empty() && g_live_pinned.empty());
}

int main()
{
    check_one_buffer<DevBuf<double>>(g_live);
    check_one_buffer<DevBuf<unsigned char>>(g_live);
    check_one_buffer<PinBuf<char>>(g_live_pinned);
    CHECK(g_live.empty() && g_live_pinned.empty());
    check_group();
    CHECK(g_live.empty() && g_live_pinned.empty());
    if (g_bad || !g_live.empty() || !g_live_pinned.empty()) { printf("devbuf: %d check(s) failed\n", g_bad); return 1; }
    printf("devbuf: OK (%ld allocations, %ld frees)\n", g_allocs, g_frees);
    return 0;
}
