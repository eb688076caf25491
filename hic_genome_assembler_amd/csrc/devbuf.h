// devbuf.h - a buffer that owns its device (or pinned host) memory and knows its capacity.  Only the HIP runtime API and
// the standard library: host code can compile and test it alone (tests/devbuf_host_check.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace hicmi {

struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void release(void* p) { (void)hipHostFree(p); }
};

// Move-only.  The capacity counts elements of T and never shrinks; growing frees first and copies nothing.
template <typename T, typename Mem = DeviceMem>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    // room for `need` elements (one when need <= 0); a failure leaves the buffer empty
    hipError_t reserve(int64_t need)
    {
        if (need <= cap_ && p_) return hipSuccess;
        reset();
        if (need <= 0) need = 1;
        void* p = nullptr;
        const hipError_t e = Mem::alloc(&p, bytes_for(need));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p); cap_ = need;
        return hipSuccess;
    }
    void reset()
    {
        if (p_) Mem::release(p_);
        p_ = nullptr; cap_ = 0;
    }
    static size_t bytes_for(int64_t need) { return (size_t)(need <= 0 ? 1 : need) * sizeof(T); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    int64_t capacity() const { return cap_; }

private:
    T* p_ = nullptr;
    int64_t cap_ = 0;
};

template <typename T>
using PinBuf = DevBuf<T, PinnedMem>;

// reserve_all(&failed_bytes, a, need_a, b, need_b, ...): every buffer of the group holds its memory afterwards, or - when
// one allocation fails - every buffer of the group is empty, *failed_bytes is the size that was refused and the error is
// returned.  A guard of "same shape and all members non-null" therefore never passes on a half-built group.
inline void reset_all() {}
template <typename B, typename... Rest>
void reset_all(B& b, int64_t, Rest&&... rest)
{
    b.reset();
    reset_all(rest...);
}

inline hipError_t reserve_all(size_t*) { return hipSuccess; }
template <typename B, typename... Rest>
hipError_t reserve_all(size_t* failed_bytes, B& b, int64_t need, Rest&&... rest)
{
    hipError_t e = b.reserve(need);
    if (e != hipSuccess) { *failed_bytes = B::bytes_for(need); reset_all(rest...); return e; }
    e = reserve_all(failed_bytes, rest...);
    if (e != hipSuccess) b.reset();
    return e;
}

}  // namespace hicmi
