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
// std::vector<Lane> and std::vector<DevBuf<...>> move their elements when they grow and can never copy one
static_assert(!std::is_copy_constructible<DevBuf<int>>::value && std::is_nothrow_move_constructible<DevBuf<int>>::value, "DevBuf moves, never copies");
}  // namespace rr
