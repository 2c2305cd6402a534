// dev_mem.h — the one owner of device memory (DevArr) and of pinned host memory (PinArr) of the host side; the only place that
// calls hipMalloc / hipFree / hipHostMalloc / hipHostFree.  A typed array with a capacity in elements, move-only, released by
// its destructor.  It never synchronises, never clears the sticky error and never logs: whoever replaces a buffer that a stream
// may still be reading drains that stream first, and whoever absorbs an out-of-memory calls hipGetLastError itself.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

template <typename T, bool Pinned>
struct MemArr {
    T *p = nullptr;
    size_t cap = 0; // elements
    MemArr() = default;
    MemArr(const MemArr &) = delete;
    MemArr &operator=(const MemArr &) = delete;
    MemArr(MemArr &&o) noexcept { swap(o); }
    MemArr &operator=(MemArr &&o) noexcept {
        if (this != &o) { reset(); swap(o); }
        return *this;
    }
    ~MemArr() { reset(); }
    void reset() {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    void swap(MemArr &o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
    // exactly n elements, always fresh (a zero-sized request still yields a non-null pointer); a failure leaves (null, 0)
    hipError_t alloc(size_t n) {
        reset();
        const size_t bytes = (n ? n : 1) * sizeof(T);
        const hipError_t e = Pinned ? hipHostMalloc((void **)&p, bytes, hipHostMallocDefault) : hipMalloc((void **)&p, bytes);
        if (e != hipSuccess) p = nullptr;
        else cap = n;
        return e;
    }
    // no-op while the array holds `need` elements; otherwise a fresh allocation: the old contents are NOT carried over
    hipError_t grow(size_t need) { return p && need <= cap ? hipSuccess : alloc(need); }
    operator T *() const { return p; }
    template <typename U> U *as() const { return (U *)p; }
};
template <typename T> using DevArr = MemArr<T, false>;
template <typename T> using PinArr = MemArr<T, true>;
using DevBuf = DevArr<unsigned char>; // untyped temporaries: alloc(bytes), as<T>()
