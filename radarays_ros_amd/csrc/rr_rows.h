// rr_rows.h -- the row scatter at the end of a staged round trip (rr_stage.h).  Plain C++, no HIP: tests/cpp/rows_check.cpp drives it on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace rr {
// n_rows rows of d_stride records of `elem` bytes at src -> the caller's rows of `stride` records at dst.  Only the records that exist
// move: those of row a below min(counts[a], d_stride); every other byte of the caller's buffer stays as it was
inline void scatter_rows(void* dst, size_t stride, const void* src, size_t d_stride, size_t elem, size_t n_rows, const uint32_t* counts)
{
    for (size_t a = 0; a < n_rows; a++)
        if (const size_t k = std::min<size_t>(counts[a], d_stride))
            std::memcpy((uint8_t*)dst + a * stride * elem, (const uint8_t*)src + a * d_stride * elem, k * elem);
}
}  // namespace rr
