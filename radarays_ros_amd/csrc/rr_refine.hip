// rr_refine.hip -- gfx950 kernels of map refinement (rr_nearest_field_device, rr_refine_poses_device; the definition is in
// include/radarays_mi355.h): for every cell of a grid map the nearest occupied cell, and point-to-point ICP of ONE scan against that table
// from very many starting states at once, one table look-up per point and iteration, all iterations inside one launch.
//
//   k_near_columns    pass A of the transform, one thread per column: an upward and a downward scan leave, per cell, the signed vertical offset
//                     dy to the column's nearest occupied cell (jy = iy + dy; a tie between above and below goes to the lower jy, dy < 0),
//                     saturated at +max_dist, in the cell's own 4 bytes of the output: no scratch.  Within a column the key of the header is
//                     monotone in |dy| first and in jy second, so the column's other occupied cells can never win
//   k_near_rows       pass B, one workgroup of kNearRowTile threads per row: the row's offsets are staged in LDS (16 bits each) between two
//                     aprons of max_dist saturated cells, so the window needs no bounds test; every cell takes the minimum 64-bit key over
//                     |dx| < max_dist of ((dx^2 + dy^2) << 32) | ((iy + dy) * width + ix + dx).  A saturated offset gives d2 >= cap2 and an
//                     index that is never looked at: the minimum is below cap2 only through a true candidate.  The row is overwritten in
//                     place; no other workgroup reads or writes it
//   k_refine          the hot path.  Lanes over points, kRefK hypotheses per wave: a wave owns kRefK consecutive hypotheses through ALL
//                     iterations of the call; their states are wave-uniform f64 (every lane holds the same value and takes the same solve).
//                     A pass walks the WHOLE scan kRefPointsTile = 64 points at a time; a point is loaded once, the next step's point is
//                     fetched under this step's arithmetic, and it serves kRefK independent 4-byte gathers.  The eight int64 sums of a
//                     hypothesis are kept per lane, reduced across the wave with 64-bit shuffles that leave the totals in every lane, and
//                     the f64 solve follows in registers.  A hypothesis never leaves its wave: no atomics, no LDS, no barrier, no
//                     accumulator anywhere; lane 0 stores one 48-byte record per hypothesis behind the last pass.  A workgroup is
//                     kRefTB / 64 such waves: kRefHypsPerGroup hypotheses
//
// Every scalar travels as a kernel argument.  No scratch memory; LDS only in k_near_rows (the staged row).
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_grid.h"
#include "rr_launch.h"
#include "rr_pose2d.h"

namespace rr {

namespace {

constexpr int kRefTB = 256;                                      // threads of a k_refine workgroup: four waves
constexpr int kRefK = 4;                                         // hypotheses a wave carries (why 4: DESIGN.md §26)
constexpr int kRefHypsPerGroup = (kRefTB / 64) * kRefK;          // 16
constexpr int kRefPointsTile = 64;                               // points a wave takes per step: one per lane
constexpr int kNearRowTile = 256;                                // threads of a k_near_rows workgroup = cells of a row per sweep
constexpr uint32_t kNearNone = 0xFFFFFFFFu;

static_assert(sizeof(rr_field_config) == 32 && sizeof(rr_icp_rec) == 48, "the grid is 32 bytes, a record 48");
static_assert(sizeof(rr_radar_point) == 24, "x and y lead a 24-byte point");

using u64 = unsigned long long;

__global__ void __launch_bounds__(256) k_near_columns(const uint8_t* __restrict__ occ, int threshold, int W, int H, int max_dist,
                                                      int32_t* __restrict__ near)
{
    const int ix = blockIdx.x * 256 + threadIdx.x;
    if (ix >= W) return;
    int d = max_dist;                                            // distance down to the nearest occupied cell at or below iy (lower jy)
#pragma unroll 8
    for (int iy = 0; iy < H; iy++) {
        d = column_step(d, occ[(size_t)iy * W + ix] >= threshold, max_dist);
        near[(size_t)iy * W + ix] = d < max_dist ? -d : max_dist;
    }
    d = max_dist;                                                // ... and up to the nearest one at or above iy
#pragma unroll 8
    for (int iy = H - 1; iy >= 0; iy--) {
        d = column_step(d, occ[(size_t)iy * W + ix] >= threshold, max_dist);
        const int lo = near[(size_t)iy * W + ix];                // <= 0, or max_dist: nothing within reach below
        if (lo == max_dist || d < -lo) near[(size_t)iy * W + ix] = d;   // a tie (d == -lo) keeps the lower jy
    }
}

__global__ void __launch_bounds__(kNearRowTile) k_near_rows(uint32_t* near, int W, int max_dist)
{
    __shared__ int16_t off[kGridMaxSide + 2 * kGridMaxDist];     // [max_dist apron][W][max_dist apron]

    const int iy = blockIdx.x;
    uint32_t* row = near + (size_t)iy * W;
    const uint32_t cap2 = (uint32_t)(max_dist * max_dist);
    for (int k = threadIdx.x; k < W + 2 * max_dist; k += kNearRowTile) {
        const int ix = k - max_dist;
        off[k] = (int16_t)((ix >= 0 && ix < W) ? (int32_t)row[ix] : max_dist);
    }
    __syncthreads();                                             // the whole row has been read: it may be overwritten
    for (int ix = threadIdx.x; ix < W; ix += kNearRowTile) {
        u64 best = ~0ull;
        const int16_t* w = off + ix + max_dist;
        const int base = iy * W + ix;
#pragma unroll 4
        for (int dx = 1 - max_dist; dx < max_dist; dx++) {
            const int dy = w[dx];
            const u64 key = ((u64)(uint32_t)(dx * dx + dy * dy) << 32) | (uint32_t)(base + dy * W + dx);
            best = min(best, key);
        }
        row[ix] = (uint32_t)(best >> 32) < cap2 ? (uint32_t)best : kNearNone;
    }
}

// k = jy * W + jx with k < 2^24 and W <= 4096, split without an integer division: (float)k is exact and the quotient estimate is off by one
// at most, which the remainder puts right.  Any other k (NONE) gives some pair that the caller does not use
__device__ inline void split_index(uint32_t k, int W, float inv_w, int* jx, int* jy)
{
    int q = (int)((float)(k & 0xFFFFFFu) * inv_w);
    int r = (int)(k & 0xFFFFFFu) - q * W;
    if (r < 0) { q -= 1; r += W; }
    if (r >= W) { q += 1; r -= W; }
    *jx = r; *jy = q;
}

__global__ void __launch_bounds__(kRefTB) k_refine(const rr_radar_point* __restrict__ points, const uint32_t* __restrict__ count, int max_points,
                                                   const double* __restrict__ init, int n_hyp, const uint32_t* __restrict__ near,
                                                   rr_field_config g, int iterations, rr_icp_rec* __restrict__ recs)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int h0 = ((int)blockIdx.x * (kRefTB / 64) + wave) * kRefK;
    if (h0 >= n_hyp) return;                                      // (the whole wave; the kernel has no barrier)
    const uint32_t total = *count, m = min(total, (uint32_t)max_points);
    const int gate2 = g.gate * g.gate;
    const float inv_w = 1.0f / (float)g.width;

    Pose2d st[kRefK];
    uint32_t flags[kRefK];
#pragma unroll
    for (int k = 0; k < kRefK; k++) {
        const size_t h = (size_t)min(h0 + k, n_hyp - 1);          // a slot past the last hypothesis repeats it and is not stored
        st[k] = { init[4 * h], init[4 * h + 1], init[4 * h + 2], init[4 * h + 3] };
        flags[k] = total > (uint32_t)max_points ? RR_ICP_TRUNCATED : 0u;
        if (icp_start(st[k])) flags[k] |= RR_ICP_DEGENERATE;
    }

    for (int it = 0; it <= iterations; it++) {
        Pose2 stf[kRefK];
        long long sum[kRefK][S_COUNT];
#pragma unroll
        for (int k = 0; k < kRefK; k++) {
            stf[k] = pose_round(st[k].c, st[k].s, st[k].tx, st[k].ty);
#pragma unroll
            for (int e = 0; e < S_COUNT; e++) sum[k][e] = 0;
        }

        float x = 0.0f, y = 0.0f;
        if ((uint32_t)lane < m) { x = points[lane].x; y = points[lane].y; }
        for (uint32_t i = lane; i < m; i += kRefPointsTile) {
            float x_next = 0.0f, y_next = 0.0f;                   // the next step's point is fetched under this step's arithmetic
            if (i + kRefPointsTile < m) { x_next = points[i + kRefPointsTile].x; y_next = points[i + kRefPointsTile].y; }
            float px[kRefK], py[kRefK];
            GridCell q[kRefK];
#pragma unroll
            for (int k = 0; k < kRefK; k++) {
                pose_move(stf[k], x, y, &px[k], &py[k]);
                q[k] = grid_cell(px[k], py[k], g);
            }
            uint32_t nk[kRefK];
#pragma unroll
            for (int k = 0; k < kRefK; k++) nk[k] = near[grid_index(q[k], g)];             // kRefK independent gathers in flight
#pragma unroll
            for (int k = 0; k < kRefK; k++) {
                int jx, jy;
                split_index(nk[k], g.width, inv_w, &jx, &jy);
                const int ddx = q[k].ix - jx, ddy = q[k].iy - jy;
                if (q[k].in && nk[k] != kNearNone && ddx * ddx + ddy * ddy <= gate2)
                    icp_accumulate(sum[k], px[k], py[k], cell_centre(g.x0, g.cell, jx), cell_centre(g.y0, g.cell, jy));
            }
            x = x_next; y = y_next;
        }

#pragma unroll
        for (int k = 0; k < kRefK; k++) {
            long long S[S_COUNT];
#pragma unroll
            for (int e = 0; e < S_COUNT; e++) S[e] = wave_sum(sum[k][e]);                  // the total in every lane
            if (it == iterations) {
                if (lane == 0 && h0 + k < n_hyp) {
                    rr_icp_rec r;
                    r.c = st[k].c; r.s = st[k].s; r.tx = st[k].tx; r.ty = st[k].ty; r.sse = S[S_SSE]; r.n_matched = (uint32_t)S[S_N]; r.flags = flags[k];
                    recs[h0 + k] = r;
                }
                continue;
            }
            if (icp_solve(S, st[k])) flags[k] |= RR_ICP_DEGENERATE;                        // the SOLVE of the scan matcher (rr_pose2d.h)
        }
    }
}

}  // namespace

void refine_tile_sizes(int* points_tile, int* hyps_per_group, int* row_tile)
{
    if (points_tile) *points_tile = kRefPointsTile;
    if (hyps_per_group) *hyps_per_group = kRefHypsPerGroup;
    if (row_tile) *row_tile = kNearRowTile;
}

void launch_nearest_field(const uint8_t* occ, int threshold, const rr_field_config& g, uint32_t* nearest, hipStream_t s)
{
    hipLaunchKernelGGL(k_near_columns, dim3((unsigned)((g.width + 255) / 256)), dim3(256), 0, s, occ, threshold, g.width, g.height, g.max_dist,
                       reinterpret_cast<int32_t*>(nearest));
    hipLaunchKernelGGL(k_near_rows, dim3((unsigned)g.height), dim3(kNearRowTile), 0, s, nearest, g.width, g.max_dist);
}

void launch_refine(const rr_radar_point* points, const uint32_t* count, int max_points, const double* init, int n_hyp, const uint32_t* nearest,
                   const rr_field_config& g, int iterations, rr_icp_rec* recs, hipStream_t s)
{
    const unsigned groups = (unsigned)((n_hyp + kRefHypsPerGroup - 1) / kRefHypsPerGroup);
    hipLaunchKernelGGL(k_refine, dim3(groups), dim3(kRefTB), 0, s, points, count, max_points, init, n_hyp, nearest, g, iterations, recs);
}

}  // namespace rr
