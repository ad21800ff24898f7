// rr_devbuf.h -- DevBuf<T>: a device buffer that only ever grows, allocated on the current device and freed with its owner (it moves, it is never
// copied).  On its own so that rr_multi.hip, which is built on the public entry points only, can use it without the context's internals (rr_ctx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <type_traits>

namespace rr {
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
    ~DevBuf() { release(); }
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }      // (for a buffer that goes before its owner does)
};
// Scratch that a device form keeps in the context, on the caller's stream s: room for n elements in each buffer named (n = 0: this call
// does not use it).  s is drained only if some buffer must grow -- an earlier call's kernels may still read what is freed then
template <class T> struct Need { DevBuf<T>& buf; size_t n; };
template <class T> Need<T> need(DevBuf<T>& buf, size_t n) { return Need<T>{ buf, n }; }
template <class... T> hipError_t grow_on_stream(hipStream_t s, Need<T>... want)
{
    hipError_t e = hipSuccess;
    if (((want.n > want.buf.n) || ...)) e = hipStreamSynchronize(s);
    ((e = e == hipSuccess && want.n ? want.buf.ensure(want.n) : e), ...);
    return e;
}
// std::vector<Lane> and std::vector<DevBuf<...>> move their elements when they grow and can never copy one
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && std::is_nothrow_move_constructible<DevBuf<int>>::value, "DevBuf moves, never copies");
}  // namespace rr
