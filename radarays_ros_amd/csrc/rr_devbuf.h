// rr_devbuf.h -- DevBuf<T>: a device buffer that only ever grows, allocated on the current device.  On its own so that
// rr_multi.hip, which is built on the public entry points only, can use it without the context's internals (rr_ctx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace rr {
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    hipError_t ensure(size_t count) {
        if (count <= n && p) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e == hipSuccess) n = count;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};
}  // namespace rr
