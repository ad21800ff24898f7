// rr_field.hip -- gfx950 kernels of the likelihood field (rr_rasterize_points_device, rr_distance_field_device, rr_score_poses_device; the
// definition is in include/radarays_mi355.h): clouds into an occupancy grid, the exact saturated squared distance transform of that grid,
// and the score of very many pose hypotheses for one scan as one table look-up per point.
//
//   k_field_raster    grid (point tiles, frames), one thread per point: the frame's state rounded to f32, the point moved into the map frame,
//                     the cell rule, and a byte 1 into the cell of a point that is IN GRID.  Every writer of a cell writes the same byte, so
//                     neither the order nor the number of writers matters
//   k_field_columns   pass A of the transform, one thread per column: an upward and a downward scan leave g[iy][ix], the vertical distance to
//                     the nearest occupied cell of the column saturated at max_dist, in the output buffer (a u16 per cell)
//   k_field_rows      pass B, one workgroup of kFieldRowTile threads per row: g * g of the row is staged in LDS between two aprons of
//                     max_dist saturated cells, so the window min over |dx| <= max_dist of dx * dx + g2[ix + dx] needs no bounds test; the
//                     row is then overwritten in place (no other workgroup reads or writes it).  Beyond the window dx * dx >= cap2 and a
//                     saturated g contributes >= cap2, so the clamped window minimum is min(cap2, the exact minimum over all occupied cells)
//   k_field_score     the hot path.  Lanes over points, kFieldK hypotheses per wave: a wave owns kFieldK consecutive hypotheses, whose states
//                     are wave-uniform, and walks the WHOLE scan kFieldPointsTile = 64 points at a time; a point is loaded once and serves
//                     kFieldK independent 2-byte gathers, which the compiler issues together.  Consecutive points of a scan are neighbours
//                     in space, so the 64 gathers of one hypothesis fall into few cache lines.  The three integer sums of a hypothesis are
//                     kept per lane (32-bit: at most 1,024 points per lane of at most 65,535 each), reduced across the wave with shuffles
//                     and stored by lane 0 as one record: a hypothesis never leaves its wave, so there are no atomics, no zeroing launch,
//                     no LDS and no barrier.  A workgroup is kFieldTB / 64 such waves: kFieldHypsPerGroup hypotheses
//
// Every scalar travels as a kernel argument.  No scratch memory; LDS only in k_field_rows (the staged row).
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_grid.h"
#include "rr_launch.h"
#include "rr_pose2d.h"

namespace rr {

namespace {

constexpr int kFieldTB = 256;                                    // threads of a k_field_score workgroup: four waves
constexpr int kFieldK = 8;                                       // hypotheses a wave scores at once (why 8: DESIGN.md §23)
constexpr int kFieldHypsPerGroup = (kFieldTB / 64) * kFieldK;    // 32
constexpr int kFieldPointsTile = 64;                             // points a wave takes per step: one per lane
constexpr int kFieldRowTile = 64;                                // threads of a k_field_rows workgroup = cells of a row per sweep

static_assert(sizeof(rr_field_config) == 32 && sizeof(rr_field_rec) == 16, "the grid is 32 bytes, a record 16");
static_assert(sizeof(rr_radar_point) == 24, "x and y lead a 24-byte point");

__global__ void __launch_bounds__(256) k_field_raster(const rr_radar_point* points, const uint32_t* offsets, int n_angles, int max_points,
                                                      const double* states, rr_field_config g, uint8_t* occ)
{
    const int f = blockIdx.y;
    const uint32_t m = frame_count(offsets, f, n_angles, max_points, nullptr);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const Pose2 st = pose_of(states, (size_t)f);
    const rr_radar_point* src = points + (size_t)f * max_points;
    float px, py;
    pose_move(st, src[i].x, src[i].y, &px, &py);
    const GridCell q = grid_cell(px, py, g);
    if (q.in) occ[grid_index(q, g)] = 1;
}

__global__ void __launch_bounds__(256) k_field_columns(const uint8_t* __restrict__ occ, int threshold, int W, int H, int max_dist,
                                                       uint16_t* __restrict__ field)
{
    const int ix = blockIdx.x * 256 + threadIdx.x;
    if (ix >= W) return;
    int d = max_dist;
#pragma unroll 8
    for (int iy = 0; iy < H; iy++) {
        d = column_step(d, occ[(size_t)iy * W + ix] >= threshold, max_dist);
        field[(size_t)iy * W + ix] = (uint16_t)d;
    }
    d = max_dist;
#pragma unroll 8
    for (int iy = H - 1; iy >= 0; iy--) {
        d = column_step(d, occ[(size_t)iy * W + ix] >= threshold, max_dist);
        field[(size_t)iy * W + ix] = (uint16_t)min((int)field[(size_t)iy * W + ix], d);
    }
}

__global__ void __launch_bounds__(kFieldRowTile) k_field_rows(uint16_t* field, int W, int max_dist)
{
    __shared__ uint16_t g2[kGridMaxSide + 2 * kGridMaxDist];   // [max_dist apron][W][max_dist apron]

    uint16_t* row = field + (size_t)blockIdx.x * W;
    const uint32_t cap2 = (uint32_t)(max_dist * max_dist);
    for (int k = threadIdx.x; k < W + 2 * max_dist; k += kFieldRowTile) {
        const int ix = k - max_dist;
        uint32_t v = cap2;
        if (ix >= 0 && ix < W) { const uint32_t g = row[ix]; v = g * g; }
        g2[k] = (uint16_t)v;                                     // (at most 255 * 255)
    }
    __syncthreads();                                             // the whole row has been read: it may be overwritten
    for (int ix = threadIdx.x; ix < W; ix += kFieldRowTile) {
        uint32_t best = cap2;
        const uint16_t* w = g2 + ix + max_dist;
#pragma unroll 4
        for (int dx = -max_dist; dx <= max_dist; dx++) best = min(best, (uint32_t)(dx * dx) + w[dx]);
        row[ix] = (uint16_t)best;
    }
}

__global__ void __launch_bounds__(kFieldTB) k_field_score(const rr_radar_point* __restrict__ points, const uint32_t* __restrict__ count,
                                                          int max_points, const float* __restrict__ states, int n_hyp,
                                                          const uint16_t* __restrict__ field, rr_field_config g, rr_field_rec* __restrict__ recs)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int h0 = ((int)blockIdx.x * (kFieldTB / 64) + wave) * kFieldK;
    if (h0 >= n_hyp) return;                                      // (the whole wave; the kernel has no barrier)
    const uint32_t m = min(*count, (uint32_t)max_points);
    const uint32_t cap2 = (uint32_t)(g.max_dist * g.max_dist), gate2 = (uint32_t)(g.gate * g.gate);

    Pose2 st[kFieldK];
    uint32_t sum[kFieldK], n_in[kFieldK], n_hit[kFieldK];
#pragma unroll
    for (int k = 0; k < kFieldK; k++) {
        const size_t h = (size_t)min(h0 + k, n_hyp - 1);          // a slot past the last hypothesis repeats it and is not stored
        st[k] = pose_of(states, h);
        sum[k] = 0; n_in[k] = 0; n_hit[k] = 0;
    }

    float x = 0.0f, y = 0.0f;
    if ((uint32_t)lane < m) { x = points[lane].x; y = points[lane].y; }
    for (uint32_t i = lane; i < m; i += kFieldPointsTile) {
        float x_next = 0.0f, y_next = 0.0f;                       // the next step's point is fetched under this step's arithmetic
        if (i + kFieldPointsTile < m) { x_next = points[i + kFieldPointsTile].x; y_next = points[i + kFieldPointsTile].y; }
        GridCell q[kFieldK];
#pragma unroll
        for (int k = 0; k < kFieldK; k++) {
            float px, py;
            pose_move(st[k], x, y, &px, &py);
            q[k] = grid_cell(px, py, g);
        }
        uint32_t d[kFieldK];
#pragma unroll
        for (int k = 0; k < kFieldK; k++) d[k] = field[grid_index(q[k], g)];      // kFieldK independent gathers in flight
#pragma unroll
        for (int k = 0; k < kFieldK; k++) {
            sum[k] += q[k].in ? d[k] : cap2;
            n_in[k] += q[k].in ? 1u : 0u;
            n_hit[k] += (q[k].in && d[k] <= gate2) ? 1u : 0u;
        }
        x = x_next; y = y_next;
    }

#pragma unroll
    for (int k = 0; k < kFieldK; k++) {
        const unsigned long long t = wave_sum((unsigned long long)sum[k]);      // the scan's total may pass 2^32
        const uint32_t in_all = wave_sum(n_in[k]), hit_all = wave_sum(n_hit[k]);
        if (lane == 0 && h0 + k < n_hyp) {
            rr_field_rec r;
            r.sum_d2 = t; r.n_in = in_all; r.n_hit = hit_all;
            recs[h0 + k] = r;                                     // one plain vector store per hypothesis
        }
    }
}

}  // namespace

void field_tile_sizes(int* points_tile, int* hyps_per_group, int* row_tile)
{
    if (points_tile) *points_tile = kFieldPointsTile;
    if (hyps_per_group) *hyps_per_group = kFieldHypsPerGroup;
    if (row_tile) *row_tile = kFieldRowTile;
}

void launch_field_raster(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points, const double* states,
                         const rr_field_config& g, uint8_t* occ, hipStream_t s)
{
    if (max_points <= 0) return;
    const dim3 grid((unsigned)((max_points + 255) / 256), (unsigned)n_frames);
    hipLaunchKernelGGL(k_field_raster, grid, dim3(256), 0, s, points, offsets, n_angles, max_points, states, g, occ);
}

void launch_distance_field(const uint8_t* occ, int threshold, const rr_field_config& g, uint16_t* field, hipStream_t s)
{
    hipLaunchKernelGGL(k_field_columns, dim3((unsigned)((g.width + 255) / 256)), dim3(256), 0, s, occ, threshold, g.width, g.height, g.max_dist, field);
    hipLaunchKernelGGL(k_field_rows, dim3((unsigned)g.height), dim3(kFieldRowTile), 0, s, field, g.width, g.max_dist);
}

void launch_field_score(const rr_radar_point* points, const uint32_t* count, int max_points, const float* states, int n_hyp, const uint16_t* field,
                        const rr_field_config& g, rr_field_rec* recs, hipStream_t s)
{
    const unsigned groups = (unsigned)((n_hyp + kFieldHypsPerGroup - 1) / kFieldHypsPerGroup);
    hipLaunchKernelGGL(k_field_score, dim3(groups), dim3(kFieldTB), 0, s, points, count, max_points, states, n_hyp, field, g, recs);
}

}  // namespace rr
