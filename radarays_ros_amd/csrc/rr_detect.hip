// rr_detect.hip -- gfx950 kernels that turn polar images into radar point clouds and Cartesian images
// (rr_detect_device / rr_polar_to_cartesian_device; the definitions are in include/radarays_mi355.h).
//
//   k_detect<TW, METHOD, false>  one workgroup per (tile of TW adjacent columns, frame): the tile is staged in LDS row by row
//                                (16-B row loads when n_angles allows, as the image lies) and read down its columns;
//                                writes each column's detection count into d_offsets
//   k_detect_scan                one wave per frame: the counts -> exclusive prefix in place, the total at [n_angles]
//   k_detect<TW, METHOD, true>   the same detections again, each written at its offset (nothing past max_points)
//   k_cartesian                  one thread per 4 output pixels, u8x4 stores; gathers from the polar image (L2 / MALL)
//
// Inside a tile a column belongs to TPC = 512 / TW consecutive threads, thread k owning the k-th contiguous chunk of bins,
// so a detection's place follows from the counts of the chunks before it: no global atomics, the output is deterministic.
// CA-CFAR keeps sliding window sums per chunk; k-strongest finds each column's threshold value from a 256-bin LDS histogram
// (two 16-bit counts per word), takes every candidate above it and the first (by bin) of those equal to it.
// Every value a call needs travels as a kernel argument; the kernels use no scratch and at most 64 KB of LDS.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_polar.h"

#include <algorithm>

namespace rr {

namespace {

constexpr int kDetTB = 512;
constexpr int kLdsMax = 65536;

struct DetectArgs {
    int method, guard, train, k, min_intensity, min_bin;
    float cfar_scale;
    PolarGrid G;
    int max_points;
    int vec;                            // rows of a tile are loaded as TW-byte words
};

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// LDS of a detect workgroup: the tile, one word per thread for the chunk prefixes, the histograms (k-strongest)
size_t detect_lds(int tw, int method, int n_cells)
{
    return align16((size_t)tw * n_cells) + 4 * kDetTB + (method == 1 ? (size_t)tw * 128 * 4 : 0);
}

template <int TW> struct RowWord;
template <> struct RowWord<16> { using T = uint4; };
template <> struct RowWord<4> { using T = uint32_t; };

// tile[r][c] = image[r][col0 + c] (0 past the last column)
template <int TW>
__device__ inline void load_tile(const uint8_t* img, uint8_t* tile, int col0, const DetectArgs& A)
{
    if (A.vec) {
        using W = typename RowWord<TW>::T;
#pragma unroll 4
        for (int r = threadIdx.x; r < A.G.n_cells; r += kDetTB)
            *reinterpret_cast<W*>(tile + (size_t)r * TW) = *reinterpret_cast<const W*>(img + (size_t)r * A.G.n_angles + col0);
    } else {            // n_angles not a multiple of TW (or an unaligned base): lanes along the row, byte loads
        for (int e = threadIdx.x; e < A.G.n_cells * TW; e += kDetTB) {
            const int r = e / TW, c = e - r * TW;
            tile[e] = col0 + c < A.G.n_angles ? img[(size_t)r * A.G.n_angles + col0 + c] : (uint8_t)0;
        }
    }
}

// the k-th chunk's exclusive prefix of v over the chunks of column c, and the column's total
__device__ inline uint32_t chunk_prefix(uint32_t* part, uint32_t v, int c, int k, int tpc, uint32_t* total)
{
    __syncthreads();                    // earlier readers of `part` are done
    part[threadIdx.x] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int q = 0; q < tpc; q++) {
        const uint32_t x = part[c * tpc + q];
        before += q < k ? x : 0u;
        all += x;
    }
    *total = all;
    return before;
}

struct Emit {
    rr_radar_point* out;                // frame's points
    uint32_t at;                        // index of this chunk's first detection in the frame
    int max_points;
    int col;
    float cs, sn;                       // direction of the column's azimuth
    const PolarGrid& G;
    __device__ void operator()(int i, int z, uint32_t nth) const
    {
        const uint32_t idx = at + nth;
        if (idx >= (uint32_t)max_points) return;
        const float r = bin_range(G, i);
        rr_radar_point p;
        p.x = r * cs; p.y = r * sn; p.z = 0.0f;
        p.intensity = (float)z;
        p.column = (uint32_t)col; p.bin = (uint32_t)i;
        out[idx] = p;
    }
};
struct NoEmit { __device__ void operator()(int, int, uint32_t) const {} };

// CA-CFAR over bins [lo, hi) of the column z(i) = tile[i * TW + c]; f(i, z, nth) per detection, bins ascending
template <int TW, class F>
__device__ inline uint32_t cfar_chunk(const uint8_t* tile, int c, int lo, int hi, const DetectArgs& A, const F& f)
{
    const int N = A.G.n_cells, G = A.guard, T = A.train;
    const int i0 = max(lo, A.min_bin);
    if (i0 >= hi) return 0;
    uint32_t sl = 0, sr = 0;
    for (int j = max(0, i0 - G - T); j <= i0 - G - 1; j++) sl += tile[j * TW + c];
    for (int j = i0 + G + 1; j <= min(N - 1, i0 + G + T); j++) sr += tile[j * TW + c];
    uint32_t cnt = 0;
    // the four cells that slide in and out are read unconditionally (clamped) and masked: the five LDS reads of a bin issue
    // together instead of one after another behind branches (measured at the target: CA-CFAR 289 us per 16-frame batch
    // that way, 181 us with the reads batched and 512 threads per workgroup instead of 256)
#pragma unroll 4
    for (int i = i0; i < hi; i++) {
        const int nl = max(0, (i - G - 1) - max(0, i - G - T) + 1);
        const int nr = max(0, min(N - 1, i + G + T) - (i + G + 1) + 1);
        const int n = nl + nr;
        const int z = tile[i * TW + c];
        const uint32_t in_l = tile[max(i - G, 0) * TW + c], out_l = tile[max(i - G - T, 0) * TW + c];
        const uint32_t out_r = tile[min(i + G + 1, N - 1) * TW + c], in_r = tile[min(i + G + T + 1, N - 1) * TW + c];
        if (z >= A.min_intensity && n > 0 && (float)(z * n) > A.cfar_scale * (float)(sl + sr)) { f(i, z, cnt); cnt++; }
        // slide to i + 1: left window [i+1-G-T, i-G], right window [i+G+2, i+G+T+1]
        sl += (i - G >= 0 ? in_l : 0u) - (i - G - T >= 0 ? out_l : 0u);
        sr += (i + G + T + 1 < N ? in_r : 0u) - (i + G + 1 < N ? out_r : 0u);
    }
    return cnt;
}

// k-strongest over bins [lo, hi): candidates above thr, and equal ones while this chunk's quota of them lasts
template <int TW, class F>
__device__ inline uint32_t kstrong_chunk(const uint8_t* tile, int c, int lo, int hi, const DetectArgs& A, int thr, int eq_quota, const F& f)
{
    uint32_t cnt = 0;
    int eq = 0;
#pragma unroll 4
    for (int i = max(lo, A.min_bin); i < hi; i++) {
        const int z = tile[i * TW + c];
        if (z < A.min_intensity) continue;
        bool take = z > thr;
        if (z == thr) { take = eq < eq_quota; eq++; }
        if (take) { f(i, z, cnt); cnt++; }
    }
    return cnt;
}

template <int TW, int METHOD, bool EMIT>
__global__ void __launch_bounds__(kDetTB) k_detect(const uint8_t* imgs, rr_radar_point* points, uint32_t* offsets, DetectArgs A)
{
    constexpr int TPC = kDetTB / TW;
    extern __shared__ __align__(16) uint8_t smem[];
    uint8_t* tile = smem;
    uint32_t* part = reinterpret_cast<uint32_t*>(smem + align16((size_t)TW * A.G.n_cells));
    uint32_t* hist = part + kDetTB;                         // [TW][128]: counts of values 2w (low half) and 2w + 1 (high half)
    __shared__ int sel_thr[TW], sel_need[TW];

    const int f = blockIdx.y;
    const int col0 = blockIdx.x * TW;
    const int c = threadIdx.x / TPC, k = threadIdx.x % TPC;
    const int col = col0 + c;
    const int chunk = (A.G.n_cells + TPC - 1) / TPC;
    const int lo = min(A.G.n_cells, k * chunk), hi = min(A.G.n_cells, lo + chunk);
    uint32_t* offs = offsets + (size_t)f * (A.G.n_angles + 1);

    load_tile<TW>(imgs + (size_t)f * A.G.n_cells * A.G.n_angles, tile, col0, A);
    int thr = 0, eq_quota = 0;
    if (METHOD == 1) {
        for (int w = threadIdx.x; w < TW * 128; w += kDetTB) hist[w] = 0;
        __syncthreads();
        uint32_t* h = hist + c * 128;
        for (int i = max(lo, A.min_bin); i < hi; i++) {
            const int z = tile[i * TW + c];
            if (z >= A.min_intensity) atomicAdd(&h[z >> 1], 1u << ((z & 1) * 16));
        }
        __syncthreads();
        if (k == 0) {
            uint32_t total = 0;
            for (int w = 0; w < 128; w++) total += (h[w] & 0xffffu) + (h[w] >> 16);
            int t = A.min_intensity - 1, need = 0;          // fewer than k candidates: every candidate
            if (total > (uint32_t)A.k) {
                uint32_t above = 0;
                for (int v = 255; v >= A.min_intensity; v--) {
                    const uint32_t n = (h[v >> 1] >> ((v & 1) * 16)) & 0xffffu;
                    if (above + n >= (uint32_t)A.k) { t = v; need = A.k - (int)above; break; }
                    above += n;
                }
            }
            sel_thr[c] = t; sel_need[c] = need;
        }
        __syncthreads();
        thr = sel_thr[c];
        // the equal cells are taken in bin order: this chunk's quota is what the chunks before it leave
        uint32_t eq_local = 0, dummy;
        if (thr >= A.min_intensity)
            for (int i = max(lo, A.min_bin); i < hi; i++) eq_local += tile[i * TW + c] == thr;
        const int eq_before = (int)chunk_prefix(part, eq_local, c, k, TPC, &dummy);
        eq_quota = max(0, sel_need[c] - eq_before);
    } else {
        __syncthreads();
    }

    const uint32_t n = METHOD == 0 ? cfar_chunk<TW>(tile, c, lo, hi, A, NoEmit{})
                                   : kstrong_chunk<TW>(tile, c, lo, hi, A, thr, eq_quota, NoEmit{});
    uint32_t col_total;
    const uint32_t before = chunk_prefix(part, n, c, k, TPC, &col_total);
    if (col >= A.G.n_angles) return;
    if (!EMIT) {
        if (k == 0) offs[col] = col_total;
        return;
    }
    if (n == 0) return;
    const float theta = az_theta(A.G, az_of_col(A.G, col));
    Emit e{ points + (size_t)f * A.max_points, offs[col] + before, A.max_points, col, cosf(theta), sinf(theta), A.G };
    if (METHOD == 0) cfar_chunk<TW>(tile, c, lo, hi, A, e);
    else kstrong_chunk<TW>(tile, c, lo, hi, A, thr, eq_quota, e);
}

// one wave per frame: counts [n_angles] -> exclusive prefix, total at [n_angles]
__global__ void __launch_bounds__(64) k_detect_scan(uint32_t* offsets, int n_angles)
{
    uint32_t* o = offsets + (size_t)blockIdx.x * (n_angles + 1);
    const int lane = threadIdx.x;
    uint32_t run = 0;
    for (int base = 0; base < n_angles; base += 64) {
        const int a = base + lane;
        const uint32_t v = a < n_angles ? o[a] : 0u;
        uint32_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (a < n_angles) o[a] = run + incl - v;
        run += __shfl(incl, 63, 64);
    }
    if (lane == 0) o[n_angles] = run;
}

template <int TW, int METHOD>
void launch_detect_tw(const uint8_t* imgs, int n_frames, rr_radar_point* points, uint32_t* offsets, const DetectArgs& A, hipStream_t s)
{
    const dim3 grid((A.G.n_angles + TW - 1) / TW, n_frames);
    const size_t lds = detect_lds(TW, METHOD, A.G.n_cells);
    hipLaunchKernelGGL((k_detect<TW, METHOD, false>), grid, dim3(kDetTB), lds, s, imgs, points, offsets, A);
    launch_detect_scan(offsets, n_frames, A.G.n_angles, s);
    if (A.max_points > 0)
        hipLaunchKernelGGL((k_detect<TW, METHOD, true>), grid, dim3(kDetTB), lds, s, imgs, points, offsets, A);
}

// ---- Cartesian ----
struct CartArgs {
    CartGrid C;
    PolarGrid G;
    int aligned;                        // the output base is 4-byte aligned
};

// pixel (i, j) from the polar image (rr_polar.h): 0 beyond the last bin
template <int INTERP>
__device__ inline uint8_t cart_pixel(const uint8_t* img, const CartArgs& A, int i, int j)
{
    const V3 p = pixel_xy(A.C, i, j);
    const float rho = sqrtf(p.x * p.x + p.y * p.y), phi = atan2f(p.y, p.x);
    float v;
    if (!range_coord(A.G, rho, &v)) return 0;
    return polar_sample<INTERP>(img, A.G, az_coord(A.G, phi), v);
}

// INTERP: 0 nearest, 1 bilinear (two kernels, so that traces and counters tell them apart)
template <int INTERP>
__global__ void __launch_bounds__(256) k_cartesian(const uint8_t* imgs, uint8_t* out, size_t total, CartArgs A)
{
    const uint32_t w = (uint32_t)A.C.width, wsq = w * w;
    const size_t npx = (size_t)A.G.n_cells * A.G.n_angles;
    for (size_t q = 4 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x); q < total; q += 4 * (size_t)gridDim.x * blockDim.x) {
        size_t f = q / wsq;
        const uint32_t rem = (uint32_t)(q - f * wsq);
        uint32_t i = rem / w, j = rem - i * w;
        uint8_t v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            v[e] = q + e < total ? cart_pixel<INTERP>(imgs + f * npx, A, (int)i, (int)j) : (uint8_t)0;
            if (++j == w) { j = 0; if (++i == w) { i = 0; f++; } }
        }
        if (A.aligned && q + 4 <= total) {
            *reinterpret_cast<uchar4*>(out + q) = make_uchar4(v[0], v[1], v[2], v[3]);
        } else {
            for (int e = 0; e < 4 && q + e < total; e++) out[q + e] = v[e];
        }
    }
}

}  // namespace

// the widest tile whose LDS fits (16 columns up to 3440 cells for k-strongest, 3952 for CA-CFAR; else 4)
static int detect_tile_width(int method, int n_cells) { return detect_lds(16, method, n_cells) + 256 <= (size_t)kLdsMax ? 16 : 4; }

void launch_detect(const uint8_t* imgs, int n_frames, const rr_detect_config& cfg, const PolarGrid& G, rr_radar_point* points, int max_points,
                   uint32_t* offsets, hipStream_t s)
{
    DetectArgs A;
    A.method = cfg.method; A.guard = cfg.guard_cells; A.train = cfg.train_cells; A.k = cfg.k;
    A.min_intensity = cfg.min_intensity; A.min_bin = cfg.min_bin; A.cfar_scale = cfg.cfar_scale;
    A.G = G;
    A.max_points = points ? max_points : 0;
    const int tw = detect_tile_width(cfg.method, G.n_cells);
    A.vec = G.n_angles % tw == 0 && reinterpret_cast<uintptr_t>(imgs) % tw == 0;
    if (tw == 16) {
        if (cfg.method == 0) launch_detect_tw<16, 0>(imgs, n_frames, points, offsets, A, s);
        else launch_detect_tw<16, 1>(imgs, n_frames, points, offsets, A, s);
    } else {
        if (cfg.method == 0) launch_detect_tw<4, 0>(imgs, n_frames, points, offsets, A, s);
        else launch_detect_tw<4, 1>(imgs, n_frames, points, offsets, A, s);
    }
}

// the scan between a count and an emit pass, for rr_window.hip too
void launch_detect_scan(uint32_t* offsets, int n_frames, int n_angles, hipStream_t s)
{
    hipLaunchKernelGGL(k_detect_scan, dim3(n_frames), dim3(64), 0, s, offsets, n_angles);
}

void launch_cartesian(const uint8_t* imgs, int n_frames, const rr_cartesian_config& cfg, const PolarGrid& G, uint8_t* out, hipStream_t s)
{
    const CartArgs A = { { cfg.width, cfg.pixel_size }, G, reinterpret_cast<uintptr_t>(out) % 4 == 0 };
    const size_t total = (size_t)n_frames * cfg.width * cfg.width;
    const size_t groups = std::min<size_t>((total + 1023) / 1024, 8192);
    if (cfg.interpolation == 0) hipLaunchKernelGGL(k_cartesian<0>, dim3((unsigned)groups), dim3(256), 0, s, imgs, out, total, A);
    else hipLaunchKernelGGL(k_cartesian<1>, dim3((unsigned)groups), dim3(256), 0, s, imgs, out, total, A);
}

}  // namespace rr
