// host_res.hpp -- owners of the host-side HIP resources of libsbx_depth: pinned memory, events, streams.  Move-only, like DevBuf
// (common.hpp); call sites pass the raw handle on with .get() (events, streams) or .p (buffers).
#pragma once
#include <utility>

#include "common.hpp"

namespace sbx {

// pinned host memory
template <class T>
struct PinnedBuf {
    T* p = nullptr;
    size_t n = 0;
    PinnedBuf() {}
    ~PinnedBuf() { release(); }
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    // grow-only: keeps the allocation when it is already large enough (the contents do not survive growing)
    void ensure(size_t count) {
        if (count <= n) return;
        release();
        SBX_HIP(hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault));
        n = count;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr; n = 0;
    }
};

// an event without timing, created on the current device when it is first asked for
struct Event {
    Event() {}
    ~Event() { if (e) (void)hipEventDestroy(e); }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    hipEvent_t get() {
        if (!e) SBX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return e;
    }

private:
    hipEvent_t e = nullptr;
};

// a non-blocking stream, created on the current device by create(); destroyed after what was queued on it has finished
struct Stream {
    Stream() {}
    ~Stream() { close(); }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { std::swap(s, o.s); return *this; }
    void create() {
        close();
        SBX_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    }
    void close() {
        if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        s = nullptr;
    }
    hipStream_t get() const { return s; }

private:
    hipStream_t s = nullptr;
};

}  // namespace sbx
