// rr_window.hip -- gfx950 kernels of the windowed CFAR detectors (rr_detect_window_device; the definition is in
// include/radarays_mi355.h): a training window over range and azimuth under CA / GO / SO, and an ordered-statistic threshold.
//
//   k_window<METHOD, false>  one workgroup of 256 threads per (strip of TC adjacent columns, frame).  The strip is walked down TR bins at
//                            a time; each step stages TR + 2 (Gr + Tr) rows by TC + 2 halo columns (wrapped mod n_angles) in LDS, zero
//                            outside the image.  Thread (c, k) owns the k-th chunk of the step's bins in column c and leaves its
//                            detections as a bit mask; writes each column's count into d_offsets and, when asked, the mask plane
//   k_detect_scan            rr_detect.hip's: the counts -> exclusive prefix in place, the total at [n_angles]
//   k_window<METHOD, true>   the same detections again, each written at its offset (nothing past max_points)
//
// Points are ordered by column, then bin, and the caller's d_offsets [n_angles + 1] is the only room between the passes, so the detections
// of one column are counted by ONE workgroup: the strip is tiled in range in time (LDS holds one step, whatever n_cells is), and the
// workgroup count grows with n_cells by narrowing the strip (16 columns up to 1024 bins, 8 up to 2048, 4 beyond), not by splitting columns.
// CA / GO / SO: per staged row the sums over the outer and the guard column window (two uint16 planes), then four sliding sums down
// the rows (outer and guard, above and below the cell); the counts are closed-form from the clipping.
// OS: f32 multiplication by a non-negative scale is monotone, so (float)z > scale * (float)v_r holds iff at least r training cells u
// satisfy scale * (float)u < (float)z.  thr[z] (built once per launch on the host: the largest such u, or -1) makes that an integer
// count of the training cells <= thr[z]: no histogram, no selection, and only candidates are counted.
// No global atomics, no inter-workgroup waiting, no scratch.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_polar.h"

#include <algorithm>

namespace rr {

namespace {

constexpr int kWinTB = 256;
constexpr int kWinMaxTC = 16;           // a chunk is at most 16 bins (pick_tile): its detections fit one uint32
constexpr int kWinMaxTR = 1024;         // a step is at most 16 bins per thread of a column

struct WinTile { int tc, tr, hr, hc, w, vec; size_t lds; };

struct WinArgs {
    int gr, hr, ga, hc;                 // guard and guard + train, in rows and in columns
    int rank, min_intensity, min_bin;
    float scale;
    PolarGrid G;
    int max_points;
    int tc, tr, w, vec;                 // the strip, the step, the staged row length, 16-byte row loads
    uint8_t* mask;                      // [n_frames][n_cells][n_angles] or null
    int16_t thr[256];                   // OS
};

__host__ __device__ inline size_t align16w(size_t x) { return (x + 15) & ~(size_t)15; }

// LDS of a workgroup: the staged rows and (CA / GO / SO) their two planes of row sums
size_t window_lds(int method, int tc, int tr, int hr, int w)
{
    const size_t rows = (size_t)tr + 2 * (size_t)hr;
    return align16w(rows * w) + (method == 3 ? 0 : rows * tc * 4);
}

// the staged column of the strip's first column: the halo, and with 16-byte loads what brings the first staged column down to a multiple of 16
__device__ inline int staged_halo(int col0, const WinArgs& A) { return A.vec ? A.hc + ((col0 - A.hc) % 16 + 16) % 16 : A.hc; }

// rows [r0 - hr, r0 + tr + hr) of the w columns from col0 - hcp on, mod n_angles; 0 outside the image
__device__ inline void stage_rows(const uint8_t* img, uint8_t* tile, int r0, int col0, int hcp, const WinArgs& A)
{
    const int N = A.G.n_cells, NA = A.G.n_angles, rows = A.tr + 2 * A.hr;
    if (A.vec) {                        // n_angles % 16 == 0, base aligned, col0 - hcp a multiple of 16: whole 16-byte words, none straddles the seam
        const int wq = A.w / 16;
        for (int e = threadIdx.x; e < rows * wq; e += kWinTB) {
            const int lr = e / wq, j = e - lr * wq, b = r0 - A.hr + lr;
            int col = (col0 - hcp + 16 * j) % NA;
            if (col < 0) col += NA;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (b >= 0 && b < N) v = *reinterpret_cast<const uint4*>(img + (size_t)b * NA + col);
            *reinterpret_cast<uint4*>(tile + (size_t)lr * A.w + 16 * j) = v;
        }
    } else {
        for (int e = threadIdx.x; e < rows * A.w; e += kWinTB) {
            const int lr = e / A.w, j = e - lr * A.w, b = r0 - A.hr + lr;
            int col = (col0 - hcp + j) % NA;
            if (col < 0) col += NA;
            tile[e] = b >= 0 && b < N ? img[(size_t)b * NA + col] : (uint8_t)0;
        }
    }
}

// per staged row and strip column: the sum over the outer column window and over the guard column window
__device__ inline void row_sums(const uint8_t* tile, uint16_t* rs_out, uint16_t* rs_in, int hcp, const WinArgs& A)
{
    const int rows = A.tr + 2 * A.hr;
    for (int e = threadIdx.x; e < rows * A.tc; e += kWinTB) {
        const int lr = e / A.tc, c = e - lr * A.tc;
        const uint8_t* p = tile + (size_t)lr * A.w + hcp + c;
        uint32_t so = 0, si = 0;
        for (int d = -A.hc; d <= A.hc; d++) so += p[d];
        for (int d = -A.ga; d <= A.ga; d++) si += p[d];
        rs_out[e] = (uint16_t)so; rs_in[e] = (uint16_t)si;
    }
}

// the training cells of bin i, by halves: counts are closed-form (rows clipped to [0, N), columns never)
struct Halves { int n_near, n_far, n_mid; };
__device__ inline Halves window_counts(int i, const WinArgs& A)
{
    const int N = A.G.n_cells, wo = 2 * A.hc + 1, wi = 2 * A.ga + 1;
    Halves h;
    h.n_near = min(i, A.hr) * wo - min(i, A.gr) * wi;
    h.n_far = min(N - 1 - i, A.hr) * wo - min(N - 1 - i, A.gr) * wi;
    h.n_mid = wo - wi;
    return h;
}

__device__ inline bool ca_test(int z, uint32_t n, uint32_t S, float scale) { return (float)((uint32_t)z * n) > scale * (float)S; }

// CA / GO / SO over bins [lo, hi) of strip column c; lr0 = the staged row of bin lo.  Bit j of the result: bin lo + j is a detection
template <int METHOD>
__device__ inline uint32_t sums_chunk(const uint8_t* tile, const uint16_t* rs_out, const uint16_t* rs_in, int c, int lo, int hi, int lr0, int hcp,
                                      const WinArgs& A)
{
    if (lo >= hi) return 0;
    const int tc = A.tc;
    // near: rows [i - hr, i - 1] (outer) and [i - gr, i - 1] (guard); far: rows [i + 1, i + hr] and [i + 1, i + gr]; rows outside the image are 0
    uint32_t on = 0, gn = 0, of = 0, gf = 0;
    for (int d = 1; d <= A.hr; d++) { on += rs_out[(lr0 - d) * tc + c]; of += rs_out[(lr0 + d) * tc + c]; }
    for (int d = 1; d <= A.gr; d++) { gn += rs_in[(lr0 - d) * tc + c]; gf += rs_in[(lr0 + d) * tc + c]; }
    uint32_t bits = 0;
    for (int i = lo; i < hi; i++) {
        const int lr = lr0 + (i - lo);
        const int z = tile[(size_t)lr * A.w + hcp + c];
        const uint32_t o_here = rs_out[lr * tc + c], g_here = rs_in[lr * tc + c];
        if (i >= A.min_bin && z >= A.min_intensity) {
            const Halves h = window_counts(i, A);
            const uint32_t s_near = on - gn, s_far = of - gf;
            bool det = false;
            if (METHOD == 0) {
                const uint32_t n = (uint32_t)(h.n_near + h.n_far + h.n_mid);
                det = n > 0 && ca_test(z, n, s_near + s_far + (o_here - g_here), A.scale);
            } else if (h.n_near + h.n_far > 0) {            // (n > 0 follows)
                bool near;
                if (h.n_near == 0) near = false;
                else if (h.n_far == 0) near = true;
                else {
                    const uint64_t a = (uint64_t)s_near * (uint32_t)h.n_far, b = (uint64_t)s_far * (uint32_t)h.n_near;
                    near = METHOD == 1 ? a >= b : a <= b;     // GO the greater mean, SO the smaller; ties to near
                }
                det = near ? ca_test(z, (uint32_t)h.n_near, s_near, A.scale) : ca_test(z, (uint32_t)h.n_far, s_far, A.scale);
            }
            bits |= det ? 1u << (i - lo) : 0u;
        }
        if (i + 1 < hi) {               // slide to i + 1
            on += o_here - rs_out[(lr - A.hr) * tc + c];
            gn += g_here - rs_in[(lr - A.gr) * tc + c];
            of += rs_out[(lr + A.hr + 1) * tc + c] - rs_out[(lr + 1) * tc + c];
            gf += rs_in[(lr + A.gr + 1) * tc + c] - rs_in[(lr + 1) * tc + c];
        }
    }
    return bits;
}

// OS over bins [lo, hi) of strip column c: a candidate counts its training cells <= thr[z]
__device__ inline uint32_t os_chunk(const uint8_t* tile, const int16_t* thr, int c, int lo, int hi, int lr0, int hcp, const WinArgs& A)
{
    const int N = A.G.n_cells;
    uint32_t bits = 0;
    for (int i = lo; i < hi; i++) {
        const int lr = lr0 + (i - lo);
        const uint8_t* centre = tile + (size_t)lr * A.w + hcp + c;
        const int z = *centre;
        if (i < A.min_bin || z < A.min_intensity) continue;
        const Halves h = window_counts(i, A);
        const int n = h.n_near + h.n_far + h.n_mid;
        const int t = thr[z];
        if (n <= 0 || t < 0) continue;
        const int r = max(1, (n * A.rank + 999) / 1000);
        int cnt = 0;
        for (int d = max(-A.hr, -i); d <= min(A.hr, N - 1 - i); d++) {
            const uint8_t* p = centre + d * A.w;
            if (d < -A.gr || d > A.gr) {
                for (int e = -A.hc; e <= A.hc; e++) cnt += p[e] <= t;
            } else {
                for (int e = A.ga + 1; e <= A.hc; e++) cnt += (p[-e] <= t) + (p[e] <= t);
            }
        }
        bits |= cnt >= r ? 1u << (i - lo) : 0u;
    }
    return bits;
}

// the k-th chunk's exclusive prefix of v over the chunks of strip column c, and the column's total
__device__ inline uint32_t chunk_prefix(uint32_t* part, uint32_t v, int c, int k, int tc, int tpc, uint32_t* total)
{
    __syncthreads();                    // earlier readers of `part` are done
    part[threadIdx.x] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int q = 0; q < tpc; q++) {
        const uint32_t x = part[q * tc + c];
        before += q < k ? x : 0u;
        all += x;
    }
    *total = all;
    return before;
}

template <int METHOD, bool EMIT>
__global__ void __launch_bounds__(kWinTB) k_window(const uint8_t* imgs, rr_radar_point* points, uint32_t* offsets, WinArgs A)
{
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ uint32_t part[kWinTB];
    __shared__ int16_t thr[256];
    const int N = A.G.n_cells, NA = A.G.n_angles, rows = A.tr + 2 * A.hr;
    uint8_t* tile = smem;                                                   // [rows][w]
    uint16_t* rs_out = reinterpret_cast<uint16_t*>(smem + align16w((size_t)rows * A.w));      // [rows][tc] each
    uint16_t* rs_in = rs_out + (size_t)rows * A.tc;

    const int f = blockIdx.y, col0 = blockIdx.x * A.tc;
    const int tpc = kWinTB / A.tc;
    const int c = threadIdx.x % A.tc, k = threadIdx.x / A.tc;               // adjacent lanes read adjacent bytes of a staged row
    const int col = col0 + c, hcp = staged_halo(col0, A);
    const int chunk = (A.tr + tpc - 1) / tpc;
    const uint8_t* img = imgs + (size_t)f * N * NA;
    uint32_t* offs = offsets + (size_t)f * (NA + 1);
    uint8_t* mask = !EMIT && A.mask ? A.mask + (size_t)f * N * NA : nullptr;
    if (METHOD == 3) thr[threadIdx.x] = A.thr[threadIdx.x];                 // (kWinTB == 256; the first stage's barrier publishes it)

    float cs = 0.0f, sn = 0.0f;
    uint32_t col_base = 0;
    if (EMIT && col < NA) {
        const float theta = az_theta(A.G, az_of_col(A.G, col));
        cs = cosf(theta); sn = sinf(theta);
        col_base = offs[col];
    }
    uint32_t col_run = 0;               // this column's detections in the steps before
    for (int r0 = 0; r0 < N; r0 += A.tr) {
        __syncthreads();                // the step before is read
        stage_rows(img, tile, r0, col0, hcp, A);
        __syncthreads();
        if (METHOD != 3) { row_sums(tile, rs_out, rs_in, hcp, A); __syncthreads(); }
        const int end = min(N, r0 + A.tr);
        const int lo = min(end, r0 + k * chunk), hi = min(end, lo + chunk);
        const int lr0 = lo - r0 + A.hr;
        uint32_t bits = 0;
        if (col < NA)
            bits = METHOD == 3 ? os_chunk(tile, thr, c, lo, hi, lr0, hcp, A) : sums_chunk<METHOD>(tile, rs_out, rs_in, c, lo, hi, lr0, hcp, A);
        uint32_t col_total;
        const uint32_t before = chunk_prefix(part, (uint32_t)__popc(bits), c, k, A.tc, tpc, &col_total);
        if (mask && col < NA)
            for (int i = lo; i < hi; i++) mask[(size_t)i * NA + col] = (bits >> (i - lo)) & 1u ? (uint8_t)255 : (uint8_t)0;
        if (EMIT && bits) {
            rr_radar_point* out = points + (size_t)f * A.max_points;
            uint32_t idx = col_base + col_run + before;
            for (uint32_t m = bits; m && idx < (uint32_t)A.max_points; m &= m - 1, idx++) {
                const int i = lo + __ffs((int)m) - 1;
                const float r = bin_range(A.G, i);
                rr_radar_point p;
                p.x = r * cs; p.y = r * sn; p.z = 0.0f;
                p.intensity = (float)tile[(size_t)(i - r0 + A.hr) * A.w + hcp + c];
                p.column = (uint32_t)col; p.bin = (uint32_t)i;
                out[idx] = p;
            }
        }
        col_run += col_total;
    }
    if (!EMIT && k == 0 && col < NA) offs[col] = col_run;
}

// The strip narrows as n_cells grows, so that the workgroup count grows with it: 16 columns up to 1024 bins, 8 up to 2048, 4 beyond.  The
// step is 16 bins per thread of a column (256 / tc threads), at most kWinMaxTR.  Both shrink until the step's LDS leaves room for two
// workgroups per CU (64 KB first: more of them); a window too large for that (near the 65,535-cell bound) takes what one workgroup may have.
// The staged row length is sized for 16-byte loads wherever n_angles allows them, whether or not the base is aligned: the tile of a
// config and shape does not depend on the buffer
bool pick_tile(int method, int hr, int hc, int n_cells, int n_angles, bool aligned, WinTile* t)
{
    const size_t budgets[3] = { 64 * 1024 - 2048, 80 * 1024 - 2048, 160 * 1024 - 2048 };
    const int tc_top = n_cells <= 1024 ? kWinMaxTC : n_cells <= 2048 ? 8 : 4;
    const bool wide = n_angles % 16 == 0;
    for (size_t budget : budgets)
        for (int tc = tc_top; tc >= 1; tc >>= 1)
            for (int tr = std::min(kWinMaxTR, 16 * (kWinTB / tc)); tr >= 32; tr >>= 1) {
                // 16-byte loads: the first staged column is the multiple of 16 at or below col0 - hc, up to 15 columns further left
                const int w_vec = tc == 16 ? 16 + 2 * ((hc + 15) / 16 * 16) : (15 + hc + tc + hc + 15) / 16 * 16, w_byte = tc + 2 * hc;
                const size_t lds = window_lds(method, tc, tr, hr, wide ? w_vec : w_byte);
                if (lds > budget) continue;
                const int vec = wide && aligned;
                *t = { tc, tr, hr, hc, vec ? w_vec : w_byte, vec, window_lds(method, tc, tr, hr, vec ? w_vec : w_byte) };
                return true;
            }
    return false;
}

template <int METHOD>
hipError_t launch_window_m(const uint8_t* imgs, int n_frames, rr_radar_point* points, uint32_t* offsets, const WinArgs& A, size_t lds, hipStream_t s)
{
    const dim3 grid((A.G.n_angles + A.tc - 1) / A.tc, n_frames);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_window<METHOD, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_window<METHOD, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_window<METHOD, false>), grid, dim3(kWinTB), lds, s, imgs, points, offsets, A);
    launch_detect_scan(offsets, n_frames, A.G.n_angles, s);
    if (A.max_points > 0) hipLaunchKernelGGL((k_window<METHOD, true>), grid, dim3(kWinTB), lds, s, imgs, points, offsets, A);
    return hipSuccess;
}

}  // namespace

bool window_tile_sizes(const rr_window_detect_config& cfg, int n_cells, int n_angles, int out[4])
{
    WinTile t;
    if (!pick_tile(cfg.method, cfg.guard_range + cfg.train_range, cfg.guard_azimuth + cfg.train_azimuth, n_cells, n_angles, true, &t)) return false;
    out[0] = t.tr; out[1] = t.tc; out[2] = t.hr; out[3] = t.hc;
    return true;
}

hipError_t launch_detect_window(const uint8_t* imgs, int n_frames, const rr_window_detect_config& cfg, const PolarGrid& G, rr_radar_point* points,
                                int max_points, uint32_t* offsets, uint8_t* mask, hipStream_t s)
{
    WinTile t;
    if (!pick_tile(cfg.method, cfg.guard_range + cfg.train_range, cfg.guard_azimuth + cfg.train_azimuth, G.n_cells, G.n_angles,
                   reinterpret_cast<uintptr_t>(imgs) % 16 == 0, &t))
        return hipErrorInvalidValue;
    WinArgs A;
    A.gr = cfg.guard_range; A.hr = t.hr; A.ga = cfg.guard_azimuth; A.hc = t.hc;
    A.rank = cfg.rank_permille; A.min_intensity = cfg.min_intensity; A.min_bin = cfg.min_bin; A.scale = cfg.scale;
    A.G = G;
    A.max_points = points ? max_points : 0;
    A.tc = t.tc; A.tr = t.tr; A.w = t.w; A.vec = t.vec;
    A.mask = mask;
    for (int z = 0; z < 256; z++) {     // thr[z]: the largest u with scale * (float)u < (float)z (a prefix of 0..255: the product is monotone in u)
        int u = -1;
        while (u < 255 && cfg.scale * (float)(u + 1) < (float)z) u++;
        A.thr[z] = (int16_t)u;
    }
    switch (cfg.method) {
    case 0: return launch_window_m<0>(imgs, n_frames, points, offsets, A, t.lds, s);
    case 1: return launch_window_m<1>(imgs, n_frames, points, offsets, A, t.lds, s);
    case 2: return launch_window_m<2>(imgs, n_frames, points, offsets, A, t.lds, s);
    default: return launch_window_m<3>(imgs, n_frames, points, offsets, A, t.lds, s);
    }
}

}  // namespace rr
