// poa_devres.h -- the owners of the engine host's device resources: a device buffer, an event, a stream, and the guard of a
// result that owns host memory.  Each frees what it holds when it leaves scope; all are move-only, so no two can hold one thing.
//
// Included after <hip/hip_runtime.h>, <string>, include/sxg_poa.h and the declaration of `int fail(int code, const std::string&)`:
// the header names the hip* calls and `fail` of the including file (tests/csrc/devres_check.cpp supplies counting stand-ins).
#pragma once

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    // at least `bytes`; a buffer that grows loses its contents (one eighth of headroom, or exactly `bytes` if that is refused)
    int ensure(size_t bytes) {
        if (bytes <= cap) return SXG_OK;
        release();
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            want = bytes;
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) { p = nullptr; return fail(SXG_E_NOMEM, "hipMalloc failed for " + std::to_string(bytes) + " bytes"); }
        cap = want;
        return SXG_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class Tp> Tp* as() const { return (Tp*)p; }
};

// an event or a stream: converts to the raw handle, so that it is passed to the hip* calls as one
template <class Raw, hipError_t (*destroy_fn)(Raw)>
struct DevHandle {
    Raw raw = nullptr;
    DevHandle() = default;
    DevHandle(const DevHandle&) = delete;
    DevHandle& operator=(const DevHandle&) = delete;
    DevHandle(DevHandle&& o) noexcept : raw(o.raw) { o.raw = nullptr; }
    DevHandle& operator=(DevHandle&& o) noexcept { if (this != &o) { destroy(); raw = o.raw; o.raw = nullptr; } return *this; }
    ~DevHandle() { destroy(); }
    void destroy() { if (raw) (void)destroy_fn(raw); raw = nullptr; }
    operator Raw() const { return raw; }
};
struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy> {
    hipError_t create() { destroy(); return hipEventCreate(&raw); }
};
struct DevStream : DevHandle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) { destroy(); return hipStreamCreateWithFlags(&raw, flags); }
};

// A result struct that owns host memory (`free_fn` is its sxg_poa_*_free): freed on every way out of the entry point that
// fills it, except the one that reaches dismiss().
template <class Out, void (*free_fn)(Out*)>
struct OutGuard {
    Out* out;
    explicit OutGuard(Out* o) : out(o) {}
    OutGuard(const OutGuard&) = delete;
    OutGuard& operator=(const OutGuard&) = delete;
    ~OutGuard() { if (out) free_fn(out); }
    void dismiss() { out = nullptr; }
};
