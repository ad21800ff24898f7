// rr_icp.hip -- gfx950 kernels of the two planar scan matchers (rr_register_points_device, rr_register_surfels_device; the definitions are in
// include/radarays_mi355.h): n source clouds registered against ONE target by ICP with a fixed iteration count.  The matcher is written once,
// as three kernel templates over a residual (rr_pose2d.h): PointResidual, point-to-point against a cloud with eight int64 sums per frame,
// and LineResidual, point-to-line against surface points with fourteen.  A residual says how a target record is staged, what a matched pair
// adds to the sums, and the solve; the search is the same code for both.
//
//   k_icp_init     one thread per frame: the initial state normalised into the frame's record (which carries the state from launch to
//                  launch), the TRUNCATED / DEGENERATE flags, the frame's sums zeroed
//   k_icp_pass     one correspondence pass.  Grid (source tiles, frames), kIcpTB threads, kIcpPPT source points per thread in registers
//                  (a source tile is kIcpSrcTile = kIcpTB * kIcpPPT points).  The target streams through LDS in tiles of kIcpTgtTile
//                  (x, y) pairs; a target that may not be a candidate, and the padding of the last pair, is staged as (+inf, +inf), so the
//                  inner loop has no branch: its d2 is +inf or NaN and `d2 < best` is false.  Every lane reads the same LDS address (a
//                  broadcast: one 16-B read is two targets for all 64 lanes) and spends it on 2 * kIcpPPT distance evaluations of
//                  8 VALU operations each (2 sub, 2 mul, 1 add, 1 compare, 2 selects: nothing fused) and one v_mov of the index per target.  A thread walks the target in
//                  ascending order with a strict `<`, so ties go to the lower index whatever the tiling.  What the residual needs of
//                  the matched target beyond (x, y) is fetched once, after the loop.  The matched pairs are quantised, the int64 sums
//                  are reduced across the wave with shuffles and lane 0 adds them to the frame's accumulator with one 64-bit vector
//                  atomic per sum: integer sums, so the order of arrival does not matter
//   k_icp_solve    one thread per frame: reads the sums, zeroes them, and either takes the residual's closed-form 2-D step in f64
//                  or, behind the last pass, writes sse and n_matched into the record
//
// The sums cross from k_icp_pass to k_icp_solve and the state from k_icp_solve to k_icp_pass at KERNEL BOUNDARIES only: the XCD L2s are
// not coherent within a launch.  Every scalar travels as a kernel argument.  No scratch memory; 8 KB of static LDS in k_icp_pass.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_pose2d.h"

#include <algorithm>

namespace rr {

namespace {

constexpr int kIcpTB = 128;                          // threads of a k_icp_pass workgroup: two waves
constexpr int kIcpPPT = 2;                           // source points a thread keeps in registers (why 2 and not more: DESIGN.md §22)
constexpr int kIcpSrcTile = kIcpTB * kIcpPPT;        // 256
constexpr int kIcpTgtTile = 1024;                    // (x, y) pairs of a target tile in LDS: 8 KB
constexpr uint32_t kIcpNone = 0xFFFFFFFFu;

static_assert(sizeof(rr_icp_rec) == 48, "a record is 48 bytes");
static_assert(sizeof(rr_radar_point) == 24, "x and y lead a 24-byte point");
static_assert(sizeof(rr_surfel) == 32, "(x, y, nx, ny) leads a 32-byte surfel");
static_assert(kIcpTgtTile % 2 == 0 && kIcpTB % 64 == 0, "targets are read in pairs, sums are reduced per wave");

template <class R>
__global__ void __launch_bounds__(256) k_icp_init(const double* init, const uint32_t* offsets, int n_angles, int max_points, const uint32_t* tgt_count,
                                                  int max_tgt, rr_icp_rec* recs, long long* acc, int n_frames)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    Pose2d st = { 1.0, 0.0, 0.0, 0.0 };
    uint32_t flags = 0;
    if (init) {
        st = { init[4 * (size_t)f], init[4 * (size_t)f + 1], init[4 * (size_t)f + 2], init[4 * (size_t)f + 3] };
        if (icp_start(st)) flags |= RR_ICP_DEGENERATE;
    }
    bool trunc;
    frame_count(offsets, f, n_angles, max_points, &trunc);
    if (trunc || *tgt_count > (uint32_t)max_tgt) flags |= RR_ICP_TRUNCATED;
    rr_icp_rec r;
    r.c = st.c; r.s = st.s; r.tx = st.tx; r.ty = st.ty; r.sse = 0; r.n_matched = 0; r.flags = flags;
    recs[f] = r;
    for (int k = 0; k < R::COUNT; k++) acc[(size_t)f * R::COUNT + k] = 0;
}

template <class R>
__global__ void __launch_bounds__(kIcpTB) k_icp_pass(const rr_radar_point* points, const uint32_t* offsets, int n_angles, int max_points,
                                                     const typename R::Target* tgt, const uint32_t* tgt_count, int max_tgt, const rr_icp_rec* recs,
                                                     float gate2, unsigned long long* acc, uint32_t* corr)
{
    __shared__ __align__(16) float2 tile[kIcpTgtTile];

    const int f = blockIdx.y;
    const uint32_t m = frame_count(offsets, f, n_angles, max_points, nullptr);
    const uint32_t i0 = blockIdx.x * (uint32_t)kIcpSrcTile;
    if (i0 >= m) return;                                          // (the whole workgroup: no barrier has been met)
    const uint32_t nt = min(*tgt_count, (uint32_t)max_tgt);
    const rr_radar_point* src = points + (size_t)f * max_points;

    const Pose2 st = pose_round(recs[f].c, recs[f].s, recs[f].tx, recs[f].ty);
    float px[kIcpPPT], py[kIcpPPT], best[kIcpPPT];
    uint32_t bj[kIcpPPT];
#pragma unroll
    for (int e = 0; e < kIcpPPT; e++) {
        const uint32_t i = i0 + (uint32_t)e * kIcpTB + threadIdx.x;
        px[e] = py[e] = __uint_as_float(0x7FC00000u);             // a slot past the count: NaN never wins and is never matched
        if (i < m) pose_move(st, src[i].x, src[i].y, &px[e], &py[e]);
        best[e] = INFINITY; bj[e] = kIcpNone;
    }

    for (uint32_t t0 = 0; t0 < nt; t0 += kIcpTgtTile) {
        const uint32_t cnt = min((uint32_t)kIcpTgtTile, nt - t0), padded = (cnt + 1u) & ~1u;
        if (t0) __syncthreads();                                  // the tile before this one has been read by every wave
        for (uint32_t k = threadIdx.x; k < padded; k += kIcpTB) {
            tile[k] = R::stage(tgt, t0 + k, k < cnt);         // (not live: the padding of the last pair)
        }
        __syncthreads();
        const float4* pairs = reinterpret_cast<const float4*>(tile);
        // four pairs per trip: their LDS reads are issued together, so a wave alone on its SIMD waits for the first of eight targets only
#pragma unroll 4
        for (uint32_t k = 0; k < padded / 2; k++) {
            const float4 q = pairs[k];
            const uint32_t j = t0 + 2 * k;
#pragma unroll
            for (int e = 0; e < kIcpPPT; e++) {
                const float dx = px[e] - q.x, dy = py[e] - q.y;
                const float d2 = dx * dx + dy * dy;
                if (d2 < best[e]) { best[e] = d2; bj[e] = j; }
            }
#pragma unroll
            for (int e = 0; e < kIcpPPT; e++) {
                const float dx = px[e] - q.z, dy = py[e] - q.w;
                const float d2 = dx * dx + dy * dy;
                if (d2 < best[e]) { best[e] = d2; bj[e] = j + 1; }
            }
        }
    }

    long long sum[R::COUNT];
#pragma unroll
    for (int k = 0; k < R::COUNT; k++) sum[k] = 0;
#pragma unroll
    for (int e = 0; e < kIcpPPT; e++) {
        const uint32_t i = i0 + (uint32_t)e * kIcpTB + threadIdx.x;
        if (i >= m) continue;
        uint32_t j = kIcpNone;
        if (R::in_range(px[e]) && R::in_range(py[e]) && bj[e] != kIcpNone && best[e] <= gate2) {
            j = bj[e];
            R::accumulate(sum, px[e], py[e], tgt, j);
        }
        if (corr) corr[(size_t)f * max_points + i] = j;
    }
#pragma unroll
    for (int k = 0; k < R::COUNT; k++) sum[k] = wave_sum(sum[k]);
    if ((threadIdx.x & 63) == 0 && sum[R::N] != 0) {
#pragma unroll
        for (int k = 0; k < R::COUNT; k++) atomicAdd(acc + (size_t)f * R::COUNT + k, (unsigned long long)sum[k]);
    }
}

template <class R>
__global__ void __launch_bounds__(256) k_icp_solve(rr_icp_rec* recs, long long* acc, int n_frames, int last)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n_frames) return;
    long long S[R::COUNT];
    for (int k = 0; k < R::COUNT; k++) { S[k] = acc[(size_t)f * R::COUNT + k]; acc[(size_t)f * R::COUNT + k] = 0; }
    rr_icp_rec* r = recs + f;
    if (last) {
        r->sse = R::sse(S);
        r->n_matched = (uint32_t)S[R::N];
        return;
    }
    if (R::solve(S, *r)) r->flags |= RR_ICP_DEGENERATE;
}

template <class R>
void launch_match(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points, const typename R::Target* tgt,
                  const uint32_t* tgt_count, int max_tgt, const double* init, float gate, int iterations, rr_icp_rec* recs, uint32_t* corr,
                  long long* acc, hipStream_t s)
{
    const float gate2 = gate * gate;
    const unsigned fgroups = (unsigned)((n_frames + 255) / 256);
    const dim3 grid((unsigned)((max_points + kIcpSrcTile - 1) / kIcpSrcTile), (unsigned)n_frames);
    unsigned long long* uacc = reinterpret_cast<unsigned long long*>(acc);
    hipLaunchKernelGGL(k_icp_init<R>, dim3(fgroups), dim3(256), 0, s, init, offsets, n_angles, max_points, tgt_count, max_tgt, recs, acc, n_frames);
    for (int it = 0; it <= iterations; it++) {
        const int last = it == iterations;
        if (grid.x) hipLaunchKernelGGL(k_icp_pass<R>, grid, dim3(kIcpTB), 0, s, points, offsets, n_angles, max_points, tgt, tgt_count, max_tgt,
                                       (const rr_icp_rec*)recs, gate2, uacc, last ? corr : nullptr);
        hipLaunchKernelGGL(k_icp_solve<R>, dim3(fgroups), dim3(256), 0, s, recs, acc, n_frames, last);
    }
}

}  // namespace

void icp_tile_sizes(int* source_tile, int* target_tile)
{
    if (source_tile) *source_tile = kIcpSrcTile;
    if (target_tile) *target_tile = kIcpTgtTile;
}

size_t icp_scratch_words(size_t n_frames) { return n_frames * PointResidual::COUNT; }
size_t line_scratch_words(size_t n_frames) { return n_frames * LineResidual::COUNT; }

void launch_icp(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points, const rr_radar_point* tgt,
                const uint32_t* tgt_count, int max_tgt, const double* init, float gate, int iterations, rr_icp_rec* recs, uint32_t* corr,
                long long* acc, hipStream_t s)
{
    launch_match<PointResidual>(points, offsets, n_frames, n_angles, max_points, tgt, tgt_count, max_tgt, init, gate, iterations, recs, corr, acc, s);
}

void launch_register_surfels(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points, const rr_surfel* tgt,
                             const uint32_t* tgt_count, int max_tgt, const double* init, float gate, int iterations, rr_icp_rec* recs,
                             uint32_t* corr, long long* acc, hipStream_t s)
{
    launch_match<LineResidual>(points, offsets, n_frames, n_angles, max_points, tgt, tgt_count, max_tgt, init, gate, iterations, recs, corr, acc, s);
}

}  // namespace rr
