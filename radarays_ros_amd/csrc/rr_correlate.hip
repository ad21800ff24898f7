// rr_correlate.hip -- gfx950 kernels of correlative scan matching (rr_field_pyramid_device, rr_correlate_scan_device; the definition is in
// include/radarays_mi355.h): the min-pyramid of a distance field, and the exact branch-and-bound search of a window of whole-cell offsets
// under n_rot anchor states for the node of smallest (score, index).
//
//   k_corr_pyramid    one launch per plane, one thread per cell: plane 0 is the field, plane h the minimum of four cells of plane h - 1 at
//                     stride 2^(h-1), cap2 beyond the edge.  Plain: it runs once per map
//   k_corr_cells      grid (point tiles, rotations), one thread per point and rotation: the anchor state applied in un-fused f32, the cell
//                     coordinate through rr_grid.h, and (bx, by) as two int16 in one word of the scratch; an unusable point gets the sentinel
//                     (-32768, -32768), which every look-up of every level reads as "beyond the grid": cap2.  The two divisions of a point
//                     happen here, once per point and rotation, never per node.  Block (0, 0) also clears the head of the scratch
//   k_corr_top        lanes over points, kCorrTopK top-level candidates of ONE row (same rotation, same oy) per wave: a point's cell is loaded
//                     once and serves kCorrTopK 2-byte gathers.  Launched twice: the first pass takes the smallest (LB, r, oy, ox) with one
//                     64-bit atomicMin per wave; the second, after the descent has fixed U, appends the candidates with LB <= U to the top list
//                     (levels == 0: takes the smallest (score, index) and counts the ties)
//   k_corr_descent    one wave: from the best top-level candidate down to level 0, the smallest of the four children each time; U and the
//                     greedy node go into the head
//   k_corr_expand     the hot path, one launch per level below the top, sized by `capacity` with the live count read on the device.  A wave
//                     owns kCorrParents wave-uniform parents; lanes over points; a point's cell is loaded once per parent and spent on its four
//                     children's gathers, all 4 * kCorrParents issued together.  The integer sums are kept per lane (32-bit: at most 1,024
//                     points per lane of at most 65,025 each), reduced with shuffles; the wave's surviving children are appended to the next
//                     list behind ONE atomicAdd per wave (level 0: one atomicMin of the packed key).  No division, no LDS, no scratch memory,
//                     no barrier; no workgroup waits for another, every loop is bounded by the count or the level
//   k_corr_finish     one wave: the winner (or, after an overflow, the greedy node) rescored on plane 0 for sum_d2, n_in and n_hit, and the
//                     record written by lane 0 as seven 16-byte vector stores
//
// The order in which survivors land in a list differs from run to run; nothing that reaches the record depends on it (counts are sums,
// the winner is a minimum).  Every scalar travels as a kernel argument.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_grid.h"
#include "rr_launch.h"
#include "rr_pose2d.h"
#include <algorithm>
#include <cstddef>

namespace rr {

namespace {

constexpr int kCorrTB = 256;                                     // threads of a workgroup of k_corr_top / k_corr_expand: four waves
constexpr int kCorrTopK = 8;                                     // top-level candidates of one row a wave bounds at once
constexpr int kCorrParents = 2;                                  // parents a wave expands at once: eight gathers in flight
constexpr int kCorrPointsTile = 64;                              // points a wave takes per step: one per lane
constexpr int kCorrMaxLevels = 8;
constexpr float kCorrCellRange = 16384.0f;                       // a point is USABLE iff |u|, |v| < this: (bx, by) fit an int16 with room for the window
constexpr uint32_t kCorrSentinel = 0x80008000u;                  // (-32768, -32768): with |offset| <= 2047 and 2^h <= 256 always left of and below the grid
constexpr unsigned long long kCorrIndexMask = 0x7FFFFFFFull;

static_assert(sizeof(rr_corr_config) == 32 && sizeof(rr_corr_rec) == 112, "the search is 32 bytes, its record seven 16-byte words");
static_assert(sizeof(rr_radar_point) == 24, "x and y lead a 24-byte point");

// the head of the scratch: what the launches of one call hand each other.  kept[h] is also the live count of the list of level h
struct CorrHead {
    uint32_t kept[kCorrMaxLevels + 1];
    uint32_t evaluated[kCorrMaxLevels + 1];
    unsigned long long top_key;                                  // min over the top level of LB << 31 | top index (row-major: r, oy, ox)
    unsigned long long best_key;                                 // min over the surviving nodes of score << 31 | node index
    unsigned long long upper;                                    // U: the greedy node's score
    int32_t g_rot, g_dx, g_dy;                                   // the greedy node
    uint32_t pad_[37];
};
constexpr size_t kCorrHeadBytes = 256;
static_assert(sizeof(CorrHead) == kCorrHeadBytes, "the head is 64 words");

// the window and the grid as the kernels take them
struct CorrShape {
    int W, H;                                                    // the grid
    int half_x, half_y, levels;
    int nx, ny;                                                  // top-level candidates per row, rows per rotation
    int n_rot, max_points, capacity;
    uint32_t cap2, gate2;
};

__device__ inline int cell_x(uint32_t c) { return (int)(int16_t)(c & 0xFFFFu); }
__device__ inline int cell_y(uint32_t c) { return (int)(int16_t)(c >> 16); }

// Q_h(x, y) of the header: cap2 where the 2^h window misses the grid, else the plane at the clamped corner.  The load is unconditional
// (cell 0 can always be read) and the selection follows it, so a wave's gathers are issued together
__device__ inline uint32_t corr_q(const uint16_t* __restrict__ plane, int x, int y, int span, const CorrShape& S)
{
    const bool out = x >= S.W || y >= S.H || x + span <= 0 || y + span <= 0;
    const uint32_t v = plane[out ? 0 : max(y, 0) * S.W + max(x, 0)];
    return out ? S.cap2 : v;
}

__device__ inline unsigned long long node_key(unsigned long long score, int r, int dx, int dy, const CorrShape& S)
{
    const unsigned long long index = ((unsigned long long)r * (2 * S.half_y + 1) + (dy + S.half_y)) * (2 * S.half_x + 1) + (dx + S.half_x);
    return score << 31 | index;
}

__global__ void __launch_bounds__(256) k_corr_pyramid(const uint16_t* __restrict__ prev, uint16_t* __restrict__ out, int W, int H, int stride,
                                                      uint32_t cap2)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t at = (size_t)y * W + x;
    uint32_t v = prev[at];
    if (stride > 0) {
        const bool xin = x + stride < W, yin = y + stride < H;
        v = min(v, xin ? (uint32_t)prev[at + stride] : cap2);
        v = min(v, yin ? (uint32_t)prev[at + (size_t)stride * W] : cap2);
        v = min(v, xin && yin ? (uint32_t)prev[at + (size_t)stride * W + stride] : cap2);
    }
    out[at] = (uint16_t)v;
}

__global__ void __launch_bounds__(256) k_corr_cells(const rr_radar_point* __restrict__ points, const uint32_t* __restrict__ count, int max_points,
                                                    const float* __restrict__ rot, rr_field_config g, uint32_t* __restrict__ head_words,
                                                    uint32_t* __restrict__ cells)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < kCorrHeadBytes / 4) {
        const int first_key = offsetof(CorrHead, top_key) / 4, end_key = offsetof(CorrHead, upper) / 4;      // the two minima start at all ones
        head_words[threadIdx.x] = ((int)threadIdx.x >= first_key && (int)threadIdx.x < end_key) ? 0xFFFFFFFFu : 0u;
    }
    const uint32_t m = min(*count, (uint32_t)max_points);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const int r = blockIdx.y;
    const Pose2 st = pose_of(rot, (size_t)r);
    float px, py;
    pose_move(st, points[i].x, points[i].y, &px, &py);
    const float u = cell_coord(px, g.x0, g.cell), v = cell_coord(py, g.y0, g.cell);
    const bool usable = fabsf(u) < kCorrCellRange && fabsf(v) < kCorrCellRange;      // (false for a NaN or an infinity)
    uint32_t c = kCorrSentinel;
    if (usable) c = ((uint32_t)(int)floorf(u) & 0xFFFFu) | ((uint32_t)(int)floorf(v) << 16);
    cells[(size_t)r * max_points + i] = c;
}

// kPrune false: the first pass, for the greedy descent's start.  true: the second, with U in the head
template <bool kPrune>
__global__ void __launch_bounds__(kCorrTB) k_corr_top(const uint32_t* __restrict__ count, const uint32_t* __restrict__ cells,
                                                      const uint16_t* __restrict__ plane, CorrShape S, CorrHead* __restrict__ head,
                                                      uint2* __restrict__ list)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int nxw = (S.nx + kCorrTopK - 1) / kCorrTopK;          // waves per row
    const int gw = (int)blockIdx.x * (kCorrTB / 64) + wave;
    if (gw >= S.n_rot * S.ny * nxw) return;                       // (the whole wave; the kernel has no barrier)
    const int row = gw / nxw, jx0 = (gw % nxw) * kCorrTopK;
    const int r = row / S.ny, jy = row % S.ny;
    const int oy = -S.half_y + (jy << S.levels), span = 1 << S.levels;
    const uint32_t m = min(*count, (uint32_t)S.max_points);
    const uint32_t* cr = cells + (size_t)r * S.max_points;

    int ox[kCorrTopK];
    uint32_t sum[kCorrTopK];
#pragma unroll
    for (int k = 0; k < kCorrTopK; k++) {
        ox[k] = -S.half_x + (min(jx0 + k, S.nx - 1) << S.levels);    // a slot past the row's end repeats its last candidate and is not counted
        sum[k] = 0;
    }
    for (uint32_t i = lane; i < m; i += kCorrPointsTile) {
        const uint32_t c = cr[i];
        const int bx = cell_x(c), by = cell_y(c);
        uint32_t q[kCorrTopK];
#pragma unroll
        for (int k = 0; k < kCorrTopK; k++) q[k] = corr_q(plane, bx + ox[k], by + oy, span, S);   // kCorrTopK independent gathers in flight
#pragma unroll
        for (int k = 0; k < kCorrTopK; k++) sum[k] += q[k];
    }

    unsigned long long t[kCorrTopK];
#pragma unroll
    for (int k = 0; k < kCorrTopK; k++) t[k] = wave_sum((unsigned long long)sum[k]);      // the scan's total may pass 2^32; in every lane

    if constexpr (!kPrune) {
        unsigned long long best = ~0ull;
#pragma unroll
        for (int k = 0; k < kCorrTopK; k++)
            if (jx0 + k < S.nx) best = min(best, t[k] << 31 | (unsigned long long)(row * S.nx + jx0 + k));
        if (lane == 0) atomicMin(&head->top_key, best);
    } else {
        const unsigned long long U = head->upper;
        uint32_t n_surv = 0;
        unsigned long long best = ~0ull;
#pragma unroll
        for (int k = 0; k < kCorrTopK; k++)
            if (jx0 + k < S.nx && t[k] <= U) {
                n_surv++;
                if (S.levels == 0) best = min(best, node_key(t[k], r, ox[k], oy, S));
            }
        if (lane != 0 || n_surv == 0) return;
        uint32_t at = atomicAdd(&head->kept[S.levels], n_surv);  // one atomic per wave that has survivors
        if (S.levels == 0) { atomicMin(&head->best_key, best); return; }
#pragma unroll
        for (int k = 0; k < kCorrTopK; k++)
            if (jx0 + k < S.nx && t[k] <= U) {
                if (at < (uint32_t)S.capacity) list[at] = make_uint2((uint32_t)r, (uint32_t)(oy + S.half_y) << 16 | (uint32_t)(ox[k] + S.half_x));
                at++;
            }
    }
}

// the four children of (ox, oy) at level h, on plane h - 1: offsets (a, b) * 2^(h-1) in the order (0,0) (1,0) (0,1) (1,1), that is by (oy, ox).
// A child that starts beyond the window is not a candidate
__device__ inline bool child_valid(int ox, int oy, int k, int stride, const CorrShape& S)
{
    return ox + (k & 1) * stride <= S.half_x && oy + (k >> 1) * stride <= S.half_y;
}

__global__ void __launch_bounds__(64) k_corr_descent(const uint32_t* __restrict__ count, const uint32_t* __restrict__ cells,
                                                     const uint16_t* __restrict__ pyramid, CorrShape S, CorrHead* __restrict__ head)
{
    const int lane = threadIdx.x;
    const uint32_t m = min(*count, (uint32_t)S.max_points);
    const unsigned long long key = head->top_key;
    const int t = (int)(key & kCorrIndexMask);
    unsigned long long lb = key >> 31;
    const int r = t / (S.ny * S.nx), jy = (t / S.nx) % S.ny, jx = t % S.nx;
    int ox = -S.half_x + (jx << S.levels), oy = -S.half_y + (jy << S.levels);
    const uint32_t* cr = cells + (size_t)r * S.max_points;
    const size_t plane_cells = (size_t)S.W * S.H;
    for (int h = S.levels; h >= 1; h--) {                         // bounded by the level
        const int stride = 1 << (h - 1);
        const uint16_t* plane = pyramid + (size_t)(h - 1) * plane_cells;
        uint32_t sum[4] = { 0, 0, 0, 0 };
        for (uint32_t i = lane; i < m; i += kCorrPointsTile) {
            const uint32_t c = cr[i];
            const int bx = cell_x(c), by = cell_y(c);
#pragma unroll
            for (int k = 0; k < 4; k++) sum[k] += corr_q(plane, bx + ox + (k & 1) * stride, by + oy + (k >> 1) * stride, stride, S);
        }
        unsigned long long best = ~0ull;
        int best_k = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long s = wave_sum((unsigned long long)sum[k]);
            if (child_valid(ox, oy, k, stride, S) && s < best) { best = s; best_k = k; }      // strict: ties go to the smaller (oy, ox)
        }
        lb = best;
        ox += (best_k & 1) * stride; oy += (best_k >> 1) * stride;
    }
    if (lane == 0) {
        head->upper = lb;
        head->g_rot = r; head->g_dx = ox; head->g_dy = oy;
        head->best_key = node_key(lb, r, ox, oy, S);
    }
}

// parents of level h (list_in, head->kept[h] of them) -> their children of level h - 1, bounded on plane h - 1
__global__ void __launch_bounds__(kCorrTB) k_corr_expand(const uint32_t* __restrict__ count, const uint32_t* __restrict__ cells,
                                                         const uint16_t* __restrict__ plane, CorrShape S, int h, CorrHead* __restrict__ head,
                                                         const uint2* __restrict__ list_in, uint2* __restrict__ list_out)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uint32_t n_live = head->kept[h];
    if (n_live > (uint32_t)S.capacity) return;                    // this level overflowed: nothing further is examined
    const uint32_t p0 = ((uint32_t)blockIdx.x * (kCorrTB / 64) + wave) * kCorrParents;
    if (p0 >= n_live) return;                                      // (the whole wave; the kernel has no barrier)
    const uint32_t m = min(*count, (uint32_t)S.max_points);
    const unsigned long long U = head->upper;
    const int stride = 1 << (h - 1);

    int pr[kCorrParents], ox[kCorrParents], oy[kCorrParents];
    const uint32_t* cr[kCorrParents];
    uint32_t sum[kCorrParents][4];
#pragma unroll
    for (int j = 0; j < kCorrParents; j++) {
        const uint2 e = list_in[min(p0 + j, n_live - 1)];         // a slot past the last parent repeats it and is not counted
        pr[j] = __builtin_amdgcn_readfirstlane((int)e.x);
        ox[j] = __builtin_amdgcn_readfirstlane((int)(e.y & 0xFFFFu)) - S.half_x;
        oy[j] = __builtin_amdgcn_readfirstlane((int)(e.y >> 16)) - S.half_y;
        cr[j] = cells + (size_t)pr[j] * S.max_points;
#pragma unroll
        for (int k = 0; k < 4; k++) sum[j][k] = 0;
    }

    for (uint32_t i = lane; i < m; i += kCorrPointsTile) {         // bounded by the count
        uint32_t c[kCorrParents];
#pragma unroll
        for (int j = 0; j < kCorrParents; j++) c[j] = cr[j][i];
        uint32_t q[kCorrParents][4];
#pragma unroll
        for (int j = 0; j < kCorrParents; j++) {
            const int x = cell_x(c[j]) + ox[j], y = cell_y(c[j]) + oy[j];
#pragma unroll
            for (int k = 0; k < 4; k++) q[j][k] = corr_q(plane, x + (k & 1) * stride, y + (k >> 1) * stride, stride, S);   // 4 * kCorrParents gathers in flight
        }
#pragma unroll
        for (int j = 0; j < kCorrParents; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) sum[j][k] += q[j][k];
    }

    unsigned long long t[kCorrParents][4];
    bool ok[kCorrParents][4];
    uint32_t n_eval = 0, n_surv = 0;
    unsigned long long best = ~0ull;
#pragma unroll
    for (int j = 0; j < kCorrParents; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            t[j][k] = wave_sum((unsigned long long)sum[j][k]);
            const bool cand = p0 + j < n_live && child_valid(ox[j], oy[j], k, stride, S);
            ok[j][k] = cand && t[j][k] <= U;                      // <=: ties reach level 0
            n_eval += cand ? 1u : 0u;
            n_surv += ok[j][k] ? 1u : 0u;
            if (h == 1 && ok[j][k]) best = min(best, node_key(t[j][k], pr[j], ox[j] + (k & 1) * stride, oy[j] + (k >> 1) * stride, S));
        }
    if (lane != 0) return;
    atomicAdd(&head->evaluated[h - 1], n_eval);
    if (n_surv == 0) return;
    uint32_t at = atomicAdd(&head->kept[h - 1], n_surv);          // one atomic per wave for the wave's survivors
    if (h == 1) { atomicMin(&head->best_key, best); return; }     // at level 0 the bound is the score
#pragma unroll
    for (int j = 0; j < kCorrParents; j++)
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (ok[j][k]) {
                if (at < (uint32_t)S.capacity)
                    list_out[at] = make_uint2((uint32_t)pr[j], (uint32_t)(oy[j] + (k >> 1) * stride + S.half_y) << 16 |
                                                                  (uint32_t)(ox[j] + (k & 1) * stride + S.half_x));
                at++;
            }
}

__global__ void __launch_bounds__(64) k_corr_finish(const uint32_t* __restrict__ count, const uint32_t* __restrict__ cells,
                                                    const uint16_t* __restrict__ field, CorrShape S, const CorrHead* __restrict__ head,
                                                    rr_corr_rec* __restrict__ rec)
{
    const int lane = threadIdx.x;
    const uint32_t m = min(*count, (uint32_t)S.max_points);
    bool overflow = false;
    for (int h = 1; h <= S.levels; h++) overflow = overflow || head->kept[h] > (uint32_t)S.capacity;
    int r = head->g_rot, dx = head->g_dx, dy = head->g_dy;
    if (!overflow) {
        const unsigned long long index = head->best_key & kCorrIndexMask;
        const unsigned long long wx = 2 * S.half_x + 1, wy = 2 * S.half_y + 1;
        dx = (int)(index % wx) - S.half_x; dy = (int)((index / wx) % wy) - S.half_y; r = (int)(index / (wx * wy));
    }
    const uint32_t* cr = cells + (size_t)r * S.max_points;
    uint32_t sum = 0, n_in = 0, n_hit = 0;
    for (uint32_t i = lane; i < m; i += kCorrPointsTile) {
        const uint32_t c = cr[i];
        const int x = cell_x(c) + dx, y = cell_y(c) + dy;
        const bool in = x >= 0 && x < S.W && y >= 0 && y < S.H;
        const uint32_t d = field[in ? y * S.W + x : 0];
        sum += in ? d : S.cap2;
        n_in += in ? 1u : 0u;
        n_hit += (in && d <= S.gate2) ? 1u : 0u;
    }
    const unsigned long long total = wave_sum((unsigned long long)sum);
    const uint32_t in_all = wave_sum(n_in), hit_all = wave_sum(n_hit);
    if (lane != 0) return;
    uint32_t w[28];
    w[0] = (uint32_t)r; w[1] = (uint32_t)dx; w[2] = (uint32_t)dy; w[3] = overflow ? RR_CORR_OVERFLOW : 0u;
    w[4] = (uint32_t)total; w[5] = (uint32_t)(total >> 32); w[6] = in_all; w[7] = hit_all;
    w[8] = (uint32_t)head->upper; w[9] = (uint32_t)(head->upper >> 32);
#pragma unroll
    for (int h = 0; h <= kCorrMaxLevels; h++) {
        // every top-level candidate is bounded, whatever the data: that count comes from the shape
        w[10 + h] = h == S.levels ? (uint32_t)(S.n_rot * S.ny * S.nx) : head->evaluated[h];
        w[19 + h] = head->kept[h];
    }
    uint4* out = reinterpret_cast<uint4*>(rec);
#pragma unroll
    for (int k = 0; k < 7; k++) out[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
}

size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
int corr_lists(int levels) { return levels < 2 ? levels : 2; }    // the levels' lists alternate between two buffers

CorrShape corr_shape(int n_rot, int max_points, const rr_field_config& g, const rr_corr_config& c)
{
    CorrShape S;
    S.W = g.width; S.H = g.height;
    S.half_x = c.half_x; S.half_y = c.half_y; S.levels = c.levels;
    const int span = 1 << c.levels;
    S.nx = (2 * c.half_x) / span + 1; S.ny = (2 * c.half_y) / span + 1;      // starts -half + j * 2^levels that do not pass +half
    S.n_rot = n_rot; S.max_points = max_points; S.capacity = c.capacity;
    S.cap2 = (uint32_t)(g.max_dist * g.max_dist); S.gate2 = (uint32_t)(g.gate * g.gate);
    return S;
}

}  // namespace

void correlate_tile_sizes(int* points_tile, int* tops_per_wave, int* parents_per_wave)
{
    if (points_tile) *points_tile = kCorrPointsTile;
    if (tops_per_wave) *tops_per_wave = kCorrTopK;
    if (parents_per_wave) *parents_per_wave = kCorrParents;
}

size_t correlate_scratch_bytes(size_t n_rot, size_t max_points, int levels, size_t capacity)
{
    return kCorrHeadBytes + align16(n_rot * max_points * sizeof(uint32_t)) + (size_t)corr_lists(levels) * align16(capacity * sizeof(uint2));
}

void launch_field_pyramid(const uint16_t* field, const rr_field_config& g, int levels, uint16_t* pyramid, hipStream_t s)
{
    const dim3 grid((unsigned)((g.width + 255) / 256), (unsigned)g.height);
    const size_t cells = (size_t)g.width * g.height;
    const uint32_t cap2 = (uint32_t)(g.max_dist * g.max_dist);
    if (field != pyramid) hipLaunchKernelGGL(k_corr_pyramid, grid, dim3(256), 0, s, field, pyramid, g.width, g.height, 0, cap2);
    for (int h = 1; h <= levels; h++)
        hipLaunchKernelGGL(k_corr_pyramid, grid, dim3(256), 0, s, pyramid + (size_t)(h - 1) * cells, pyramid + (size_t)h * cells, g.width, g.height,
                           1 << (h - 1), cap2);
}

void launch_correlate(const rr_radar_point* points, const uint32_t* count, int max_points, const float* rot, int n_rot, const uint16_t* pyramid,
                      const rr_field_config& g, const rr_corr_config& c, rr_corr_rec* rec, void* scratch, hipStream_t s)
{
    const CorrShape S = corr_shape(n_rot, max_points, g, c);
    uint8_t* base = static_cast<uint8_t*>(scratch);
    CorrHead* head = reinterpret_cast<CorrHead*>(base);
    uint32_t* cells = reinterpret_cast<uint32_t*>(base + kCorrHeadBytes);
    uint8_t* lists = base + kCorrHeadBytes + align16((size_t)n_rot * max_points * sizeof(uint32_t));
    const size_t list_bytes = align16((size_t)c.capacity * sizeof(uint2));
    auto list_of = [&](int h) { return reinterpret_cast<uint2*>(lists + (size_t)((c.levels - h) & 1) * list_bytes); };     // the top list is buffer 0
    const size_t plane_cells = (size_t)g.width * g.height;
    const int waves_per_group = kCorrTB / 64;

    const dim3 cell_grid((unsigned)std::max(1, (max_points + 255) / 256), (unsigned)n_rot);
    hipLaunchKernelGGL(k_corr_cells, cell_grid, dim3(256), 0, s, points, count, max_points, rot, g, reinterpret_cast<uint32_t*>(head), cells);

    const int top_waves = n_rot * S.ny * ((S.nx + kCorrTopK - 1) / kCorrTopK);
    const dim3 top_grid((unsigned)((top_waves + waves_per_group - 1) / waves_per_group));
    const uint16_t* top_plane = pyramid + (size_t)c.levels * plane_cells;
    uint2* top_list = c.levels ? list_of(c.levels) : nullptr;
    hipLaunchKernelGGL(k_corr_top<false>, top_grid, dim3(kCorrTB), 0, s, count, cells, top_plane, S, head, top_list);
    hipLaunchKernelGGL(k_corr_descent, dim3(1), dim3(64), 0, s, count, cells, pyramid, S, head);
    hipLaunchKernelGGL(k_corr_top<true>, top_grid, dim3(kCorrTB), 0, s, count, cells, top_plane, S, head, top_list);

    const int parents_per_group = waves_per_group * kCorrParents;
    const dim3 level_grid((unsigned)((c.capacity + parents_per_group - 1) / parents_per_group));      // sized by capacity: the live count is the device's
    for (int h = c.levels; h >= 1; h--)
        hipLaunchKernelGGL(k_corr_expand, level_grid, dim3(kCorrTB), 0, s, count, cells, pyramid + (size_t)(h - 1) * plane_cells, S, h, head,
                           list_of(h), h > 1 ? list_of(h - 1) : nullptr);
    hipLaunchKernelGGL(k_corr_finish, dim3(1), dim3(64), 0, s, count, cells, pyramid, S, head, rec);
}

}  // namespace rr
