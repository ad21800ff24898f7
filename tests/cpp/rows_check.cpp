// scatter_rows (csrc/rr_rows.h), the one piece of pure host logic in a staged round trip (rr_stage.h), under AddressSanitizer + UBSan:
// only the first min(count, d_stride) records of each row reach the caller; every other byte of the caller's buffer keeps its guard pattern.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I radarays_ros_amd/csrc tests/cpp/rows_check.cpp -o /tmp/rows_check && /tmp/rows_check
#include <rr_rows.h>

#include <cstdio>
#include <vector>

static const uint8_t kGuard = 0xA5;

// one case: rows of d_stride records of `elem` bytes into the caller's rows of `stride` records.  The source bytes are all different from
// the guard, so a byte that moved is a byte that changed
static int run(const char* what, size_t elem, size_t d_stride, size_t stride, const std::vector<uint32_t>& counts)
{
    const size_t n = counts.size();
    // exactly sized on both sides: a read past the staged rows or a write past the caller's is the sanitizer's to report
    std::vector<uint8_t> src(n * d_stride * elem), dst(n * stride * elem, kGuard);
    for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)(i % 160);          // 0..159: never 0xA5
    rr::scatter_rows(dst.data(), stride, src.data(), d_stride, elem, n, counts.data());
    int bad = 0;
    for (size_t a = 0; a < n && !bad; a++) {
        const size_t k = std::min<size_t>(counts[a], d_stride) * elem;
        for (size_t b = 0; b < stride * elem && !bad; b++) {
            const uint8_t got = dst[a * stride * elem + b], want = b < k ? src[a * d_stride * elem + b] : kGuard;
            if (got != want) { std::printf("%s: row %zu byte %zu is %u, expected %u\n", what, a, b, got, want); bad = 1; }
        }
    }
    return bad;
}

int main()
{
    int fails = 0;
    for (size_t elem : { (size_t)1, (size_t)4, (size_t)12, (size_t)48 }) {
        fails += run("one row, count 0", elem, 5, 5, { 0 });
        fails += run("one row, below the stride", elem, 5, 5, { 4 });
        fails += run("one row, equal to the stride", elem, 5, 5, { 5 });
        fails += run("one row, above the stride", elem, 5, 5, { 6 });
        fails += run("one row, far above the stride", elem, 5, 9, { 0xFFFFFFFFu });
        fails += run("many rows, equal strides", elem, 4, 4, { 0, 3, 4, 5, 0, 1, 4000000000u, 2 });
        fails += run("many rows, a caller stride larger than the device stride", elem, 3, 7, { 2, 0, 3, 4, 7, 8, 1, 0, 0, 3 });
        fails += run("many rows, every count 0", elem, 3, 7, { 0, 0, 0, 0 });
        fails += run("a device stride of one record", elem, 1, 6, { 0, 1, 2 });
        fails += run("no rows", elem, 3, 3, {});
    }
    std::printf("%s\n", fails ? "rows_check: FAILED" : "rows_check: ok");
    return fails ? 1 : 0;
}
