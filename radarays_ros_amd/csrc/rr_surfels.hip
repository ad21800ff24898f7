// rr_surfels.hip -- gfx950 kernels of the oriented surface points (rr_surface_points_device).  The definition is in include/radarays_mi355.h:
// integer sums, so no execution order can change a byte.
//
// Surface points, a memset of the sums and four launches:
//   k_sf_bin       one thread per point: the point's cell and its six int64 sums, one 64-bit vector atomic per sum into the cell's own row
//   k_sf_decide    a launch of its own: the launch boundary before it makes every sum of k_sf_bin visible (the XCD L2s are not coherent
//                  within a launch, so there is no last-block hand-off).  A workgroup takes a chunk of kSfChunk cells, kSfPer consecutive
//                  cells per thread: a cell that holds a point gathers the 3 x 3 block around it, shifts the neighbours' sums to its own
//                  origin in integers and takes the eigen step in f64; the keep flags go to the flag plane (four bytes per thread, one
//                  store), the number kept in the chunk to the partials
//   k_sf_offsets   one workgroup per frame: the exclusive scan of the chunks' numbers in place, the frame's total and flags to d_counts
//                  (the shape of the scan of rr_components.hip: per-chunk numbers, one workgroup over them, ranks per chunk again)
//   k_sf_write     per chunk again: every kept cell's rank in ascending cell order; a cell whose rank is below max_surfels takes the
//                  same steps again (a few hundred cells of a million: cheaper than a record per cell in the scratch) and writes its
//                  record in two 16-B stores
//
// The point-to-line matcher that takes these records as its target is rr_icp.hip's, with LineResidual of rr_pose2d.h.
// No scratch (private) memory; 32 bytes of static LDS in the scan kernels.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_pose2d.h"

#include <algorithm>

namespace rr {

namespace {

// ---- surface points ----------------------------------------------------------------------------------------------------------------
constexpr int kSfTB = 256;                          // threads of a workgroup of every kernel of this part (block_excl_scan: four waves)
constexpr int kSfPer = 4;                           // consecutive cells of a thread of k_sf_decide / k_sf_write: one word of flags
constexpr int kSfChunk = kSfTB * kSfPer;            // cells of a chunk of the scan
constexpr int kSfSums = 6;                          // N, Sx, Sy, Sxx, Sxy, Syy
constexpr float kSfRange = 8192.0f;

static_assert(sizeof(rr_surfel) == 32 && sizeof(rr_surfel_config) == 32, "a record and a config are 32 bytes");

struct SfArgs {
    int width, cell_q, half;                        // half = (width * cell_q) / 2
    uint32_t n_cells, n_chunks;                     // width * width <= 2^20; chunks of kSfChunk cells
    uint32_t min_points, max_surfels;
    double max_ratio;
};

__device__ inline int floor_div(int a, int b) { const int q = a / b; return (a % b != 0 && a < 0) ? q - 1 : q; }      // b > 0

__global__ void __launch_bounds__(kSfTB) k_sf_bin(const rr_radar_point* points, const uint32_t* offsets, int n_angles, int max_points,
                                                  unsigned long long* sums, SfArgs A)
{
    const int f = blockIdx.y;
    const uint32_t m = frame_count(offsets, f, n_angles, max_points, nullptr);
    const uint32_t i = blockIdx.x * (uint32_t)kSfTB + threadIdx.x;
    if (i >= m) return;
    const rr_radar_point* p = points + (size_t)f * max_points + i;
    const float x = p->x, y = p->y;
    if (!(fabsf(x) < kSfRange && fabsf(y) < kSfRange)) return;    // false for NaN and infinities
    const int U = (int32_t)rintf(x * 256.0f) + A.half, V = (int32_t)rintf(y * 256.0f) + A.half;
    const int ix = floor_div(U, A.cell_q), iy = floor_div(V, A.cell_q);
    if (ix < 0 || ix >= A.width || iy < 0 || iy >= A.width) return;
    const unsigned long long rx = (unsigned long long)(U - ix * A.cell_q), ry = (unsigned long long)(V - iy * A.cell_q);
    unsigned long long* s = sums + ((size_t)f * A.n_cells + (size_t)iy * A.width + ix) * kSfSums;
    atomicAdd(s + 0, 1ull);
    atomicAdd(s + 1, rx); atomicAdd(s + 2, ry);
    atomicAdd(s + 3, rx * rx); atomicAdd(s + 4, rx * ry); atomicAdd(s + 5, ry * ry);
}

// the surface point of cell `cell` of a frame whose sums start at `sums`: false if the cell holds no point or the keep rule drops it
__device__ inline bool surfel_of(const long long* sums, uint32_t cell, const SfArgs& A, rr_surfel* out)
{
    if (cell >= A.n_cells || sums[(size_t)cell * kSfSums] == 0) return false;
    const int ix = (int)(cell % (uint32_t)A.width), iy = (int)(cell / (uint32_t)A.width);
    long long N = 0, Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0;
    for (int b = -1; b <= 1; b++) {
        const int jy = iy + b;
        if (jy < 0 || jy >= A.width) continue;
        for (int a = -1; a <= 1; a++) {
            const int jx = ix + a;
            if (jx < 0 || jx >= A.width) continue;
            const long long* s = sums + ((size_t)jy * A.width + jx) * kSfSums;
            const long long n = s[0];
            if (n == 0) continue;
            const long long sx = s[1], sy = s[2], sxx = s[3], sxy = s[4], syy = s[5];
            const long long ox = (long long)a * A.cell_q, oy = (long long)b * A.cell_q;
            N += n;
            Sx += sx + n * ox; Sy += sy + n * oy;
            Sxx += sxx + 2 * ox * sx + n * ox * ox;
            Sxy += sxy + ox * sy + oy * sx + n * ox * oy;
            Syy += syy + 2 * oy * sy + n * oy * oy;
        }
    }
    const long long Cxx = N * Sxx - Sx * Sx, Cxy = N * Sxy - Sx * Sy, Cyy = N * Syy - Sy * Sy;
    const double T = (double)(Cxx + Cyy), d = (double)(Cxx - Cyy), o = (double)(2 * Cxy);
    const double h = sqrt(d * d + o * o);
    const double lmax = (T + h) / 2.0, v = (T - h) / 2.0, lmin = v > 0.0 ? v : 0.0;
    if (!((unsigned long long)N >= A.min_points && h > 0.0 && lmin <= A.max_ratio * lmax)) return false;
    if (!out) return true;
    double tx, ty;
    if (d >= 0.0) { tx = h + d; ty = o; } else { tx = o; ty = h - d; }
    const double tn = sqrt(tx * tx + ty * ty);
    tx = tx / tn; ty = ty / tn;
    const double mx = (double)(ix * A.cell_q - A.half) + (double)Sx / (double)N;
    const double my = (double)(iy * A.cell_q - A.half) + (double)Sy / (double)N;
    double nx = -ty, ny = tx;
    if (nx * mx + ny * my > 0.0) { nx = -nx; ny = -ny; }
    const double den = ((double)N * (double)N) * 65536.0;
    out->x = (float)(mx / 256.0); out->y = (float)(my / 256.0);
    out->nx = (float)nx; out->ny = (float)ny;
    out->var_n = (float)(lmin / den); out->var_t = (float)(lmax / den);
    out->count = (uint32_t)N; out->cell = cell;
    return true;
}

__global__ void __launch_bounds__(kSfTB) k_sf_decide(const long long* sums, uint32_t* flags, uint32_t* partials, SfArgs A)
{
    __shared__ int s_scan[8];
    const long long* fs = sums + (size_t)blockIdx.y * A.n_cells * kSfSums;
    const uint32_t c0 = blockIdx.x * (uint32_t)kSfChunk + threadIdx.x * kSfPer;
    uint32_t word = 0;
    int nk = 0;
#pragma unroll 1
    for (int e = 0; e < kSfPer; e++)
        if (surfel_of(fs, c0 + e, A, nullptr)) { word |= 1u << (8 * e); nk++; }
    flags[((size_t)blockIdx.y * A.n_chunks + blockIdx.x) * kSfTB + threadIdx.x] = word;
    int total;
    block_excl_scan(nk, total, s_scan);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * A.n_chunks + blockIdx.x] = (uint32_t)total;
}

__global__ void __launch_bounds__(kSfTB) k_sf_offsets(uint32_t* partials, const uint32_t* offsets, int n_angles, int max_points, uint32_t* counts, SfArgs A)
{
    __shared__ int s_scan[8];
    uint32_t* part = partials + (size_t)blockIdx.x * A.n_chunks;
    int carry = 0;
    for (uint32_t b0 = 0; b0 < A.n_chunks; b0 += kSfTB) {           // (the bound is the same in every thread: the barriers inside are met by all)
        const uint32_t b = b0 + threadIdx.x;
        const int k = b < A.n_chunks ? (int)part[b] : 0;
        int tk;
        const int ex = block_excl_scan(k, tk, s_scan);
        if (b < A.n_chunks) part[b] = (uint32_t)(carry + ex);
        carry += tk;
    }
    if (threadIdx.x == 0) {
        bool trunc;
        frame_count(offsets, blockIdx.x, n_angles, max_points, &trunc);
        counts[2 * blockIdx.x] = (uint32_t)carry;
        counts[2 * blockIdx.x + 1] = (trunc ? RR_SURFELS_TRUNCATED : 0u) | ((uint32_t)carry > A.max_surfels ? RR_SURFELS_CAPPED : 0u);
    }
}

__global__ void __launch_bounds__(kSfTB) k_sf_write(const long long* sums, const uint32_t* flags, const uint32_t* partials, rr_surfel* surfels, SfArgs A)
{
    __shared__ int s_scan[8];
    const long long* fs = sums + (size_t)blockIdx.y * A.n_cells * kSfSums;
    const uint32_t c0 = blockIdx.x * (uint32_t)kSfChunk + threadIdx.x * kSfPer;
    const uint32_t word = flags[((size_t)blockIdx.y * A.n_chunks + blockIdx.x) * kSfTB + threadIdx.x];
    const int nk = __popc(word);
    int total;
    uint32_t rank = partials[(size_t)blockIdx.y * A.n_chunks + blockIdx.x] + (uint32_t)block_excl_scan(nk, total, s_scan);
#pragma unroll 1
    for (int e = 0; e < kSfPer; e++) {
        if (!(word >> (8 * e) & 1u)) continue;
        if (rank < A.max_surfels) {
            rr_surfel r;
            surfel_of(fs, c0 + e, A, &r);
            uint4* o = reinterpret_cast<uint4*>(surfels + (size_t)blockIdx.y * A.max_surfels + rank);
            o[0] = make_uint4(__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.nx), __float_as_uint(r.ny));
            o[1] = make_uint4(__float_as_uint(r.var_n), __float_as_uint(r.var_t), r.count, r.cell);
        }
        rank++;
    }
}

SfArgs sf_args(const rr_surfel_config& g, int max_surfels)
{
    SfArgs A;
    A.width = g.width; A.cell_q = (int)rintf(g.cell * 256.0f); A.half = (A.width * A.cell_q) / 2;
    A.n_cells = (uint32_t)g.width * (uint32_t)g.width;
    A.n_chunks = (A.n_cells + kSfChunk - 1) / kSfChunk;
    A.min_points = (uint32_t)g.min_points; A.max_surfels = (uint32_t)max_surfels;
    A.max_ratio = (double)g.max_ratio;
    return A;
}

// the scratch: the sums [n][cells][6] int64 | the flag words [n][chunks][kSfTB] | the partials [n][chunks], each a multiple of 16 bytes
size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
size_t sf_sums_bytes(size_t n, size_t cells) { return align16(n * cells * kSfSums * sizeof(long long)); }
size_t sf_flags_bytes(size_t n, size_t chunks) { return align16(n * chunks * kSfTB * sizeof(uint32_t)); }
size_t sf_part_bytes(size_t n, size_t chunks) { return align16(n * chunks * sizeof(uint32_t)); }

}  // namespace

void surfels_tile_sizes(int* points_tile, int* cells_chunk)
{
    if (points_tile) *points_tile = kSfTB;
    if (cells_chunk) *cells_chunk = kSfChunk;
}

size_t surfels_scratch_bytes(size_t n_frames, size_t n_cells)
{
    const size_t chunks = (n_cells + kSfChunk - 1) / kSfChunk;
    return sf_sums_bytes(n_frames, n_cells) + sf_flags_bytes(n_frames, chunks) + sf_part_bytes(n_frames, chunks);
}

hipError_t launch_surface_points(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points,
                                 const rr_surfel_config& cfg, rr_surfel* surfels, int max_surfels, uint32_t* counts, void* scratch, hipStream_t s)
{
    const SfArgs A = sf_args(cfg, max_surfels);
    const size_t n = (size_t)n_frames;
    uint8_t* base = static_cast<uint8_t*>(scratch);
    long long* sums = reinterpret_cast<long long*>(base);
    uint32_t* flags = reinterpret_cast<uint32_t*>(base + sf_sums_bytes(n, A.n_cells));
    uint32_t* partials = reinterpret_cast<uint32_t*>(base + sf_sums_bytes(n, A.n_cells) + sf_flags_bytes(n, A.n_chunks));
    const hipError_t e = hipMemsetAsync(sums, 0, n * A.n_cells * kSfSums * sizeof(long long), s);
    if (e != hipSuccess) return e;
    const dim3 pgrid((unsigned)((max_points + kSfTB - 1) / kSfTB), (unsigned)n_frames), cgrid(A.n_chunks, (unsigned)n_frames);
    if (pgrid.x) hipLaunchKernelGGL(k_sf_bin, pgrid, dim3(kSfTB), 0, s, points, offsets, n_angles, max_points, reinterpret_cast<unsigned long long*>(sums), A);
    hipLaunchKernelGGL(k_sf_decide, cgrid, dim3(kSfTB), 0, s, (const long long*)sums, flags, partials, A);
    hipLaunchKernelGGL(k_sf_offsets, dim3((unsigned)n_frames), dim3(kSfTB), 0, s, partials, offsets, n_angles, max_points, counts, A);
    if (max_surfels > 0)
        hipLaunchKernelGGL(k_sf_write, cgrid, dim3(kSfTB), 0, s, (const long long*)sums, (const uint32_t*)flags, (const uint32_t*)partials, surfels, A);
    return hipSuccess;
}

}  // namespace rr
