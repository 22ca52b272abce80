// sgs_own.h — host side only: the owners of everything sgs_api.hip takes from the HIP runtime.  Device and pinned arrays, events and
// streams are allocated, grown and released HERE and nowhere else; what holds one is released when it goes out of scope, so no error
// path and no destroy function lists buffers by hand.  Nothing a kernel sees is declared here: kernels take the raw pointers (.p).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace sgs {

enum class Grow {
    exact,          // to the size asked for (a lane's intermediates, the mesh path's: sized by the scene and the frame)
    geometric       // to max(asked, 2 x capacity) (the encoders' and the resize's scratch: sized by the caller's batch)
};

struct DeviceMem {
    static hipError_t take(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void give(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t take(void** p, size_t bytes) { return hipHostMalloc(p, bytes, 0); }
    static void give(void* p) { (void)hipHostFree(p); }
};

// An array of `cap` elements at `p`.  INVARIANT: cap == 0 whenever p == nullptr — a capacity never outlives its array, so "is it large
// enough" is one comparison and a failed growth leaves an empty buffer that the next call grows again.
template <class T, class Mem>
struct Buf {
    T* p = nullptr;
    int64_t cap = 0;

    Buf() = default;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { reset(); }

    // (releasing device memory waits for the work that still uses it)
    void reset() {
        if (p) Mem::give(p);
        p = nullptr; cap = 0;
    }
    bool holds(int64_t want) const { return want <= cap; }
    // At least `want` elements; the contents do not survive a growth.  Nothing is asked of the runtime when the array is large enough.
    // grow(0) of an empty buffer allocates nothing and leaves it empty (there is no "a count of 0 means 1" rule here): a caller whose
    // count can be 0 and whose kernels want a pointer all the same asks for max(count, 1), as the mesh path does.
    hipError_t grow(int64_t want, Grow policy = Grow::exact) {
        if (want <= cap) return hipSuccess;
        const int64_t c = policy == Grow::geometric ? std::max<int64_t>(want, 2 * cap) : want;
        reset();
        void* q = nullptr;
        const hipError_t e = Mem::take(&q, (size_t)c * sizeof(T));
        if (e != hipSuccess) return e;
        p = static_cast<T*>(q); cap = c;
        return hipSuccess;
    }
};
template <class T> using DevBuf = Buf<T, DeviceMem>;
template <class T> using PinnedBuf = Buf<T, PinnedMem>;

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    hipError_t create() { return e ? hipSuccess : hipEventCreate(&e); }
    hipError_t create(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    hipError_t create(unsigned flags) { return s ? hipSuccess : hipStreamCreateWithFlags(&s, flags); }
};

}  // namespace sgs
