// rr_deskew.hip -- gfx950 kernels that take the motion and Doppler distortion of a sweep out again (rr_sweep_table_device /
// rr_compensate_points_device / rr_polar_to_cartesian_sweep_device; the definitions are in include/radarays_mi355.h).
//
//   k_sweep_table           one thread per (frame, azimuth): the azimuth's pose relative to the reference pose and the range
//                           shift a static world gets there, one rr_sweep_rec (two 16-B stores)
//   k_compensate_points     one thread per written point: the point's range corrected, then moved into the reference frame;
//                           reads the frame's count on the device, in place or not
//   k_cartesian_sweep       one thread per 4 output pixels, u8x4 stores, as rr_detect.hip's k_cartesian; the frame's records
//                           are staged once per workgroup in LDS (16-B loads), so the dependent table reads of the per-pixel
//                           azimuth iteration cost LDS latency, and the four pixels of a thread step through the iteration
//                           side by side (four independent LDS reads in flight).  The gathers from the polar image follow
//                           the last iteration, all of a pixel's together
//
// All f32 with nothing fused, the quaternion algebra through rr_device.h.  Every value a call needs but the table and the
// images travels as a kernel argument; the kernels use no scratch and at most 64 KB of dynamic LDS (n_angles * 32 bytes).
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_polar.h"

#include <algorithm>

namespace rr {

namespace {

static_assert(sizeof(rr_sweep_rec) == 32, "a record is two float4");

struct SweepRec { Quat q; V3 t; float dr; };

__device__ inline SweepRec rec_of(float4 a, float4 b) { return { { a.x, a.y, a.z, a.w }, { b.x, b.y, b.z }, b.w }; }

// ---- the table ----
__global__ void __launch_bounds__(256) k_sweep_table(const float* az_poses, const float* ref_poses, const float* vel, float gain, PolarGrid G,
                                                     size_t total, float4* table)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t f = e / (size_t)G.n_angles;
        const int a = (int)(e - f * (size_t)G.n_angles);
        const float* pa = az_poses + 7 * e;
        const float* pr = ref_poses + 7 * f;
        const Quat q_a = { pa[0], pa[1], pa[2], pa[3] }, q_ref = { pr[0], pr[1], pr[2], pr[3] };
        const V3 t_a = { pa[4], pa[5], pa[6] }, t_ref = { pr[4], pr[5], pr[6] };
        const Quat q = q_mul(q_conj(q_ref), q_a);
        const V3 t = q_rot(q_conj(q_ref), v_sub(t_a, t_ref));
        float dr = 0.0f;
        if (vel && gain != 0.0f) {
            const float theta = az_theta(G, a);
            const V3 u = q_rot(q_a, V3{ cosf(theta), sinf(theta), 0.0f });
            const V3 v_s = { vel[3 * f], vel[3 * f + 1], vel[3 * f + 2] };
            const float v_r = -(v_dot(v_s, u));
            dr = gain * v_r;
        }
        table[2 * e] = make_float4(q.x, q.y, q.z, q.w);
        table[2 * e + 1] = make_float4(t.x, t.y, t.z, dr);
    }
}

// ---- points ----
__global__ void __launch_bounds__(256) k_compensate_points(const rr_radar_point* points, const uint32_t* offsets, int max_points, const float4* table,
                                                           rr_radar_point* out, PolarGrid G)
{
    const int f = blockIdx.y, n_angles = G.n_angles;
    const uint32_t total = offsets[(size_t)f * (n_angles + 1) + n_angles];
    const uint32_t m = min(total, (uint32_t)max_points);
    const size_t base = (size_t)f * max_points;
    const float4* tab = table + 2 * (size_t)f * n_angles;
    const float nan = __uint_as_float(0x7FC00000u);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        rr_radar_point p = points[base + i];
        V3 o = { nan, nan, nan };
        if (p.column < (uint32_t)n_angles) {                 // (a point that is not one of this shape has no azimuth)
            const int a = az_of_col(G, (int)p.column);
            const SweepRec rec = rec_of(tab[2 * a], tab[2 * a + 1]);
            const float r = bin_range(G, p.bin);
            const float rc = r - rec.dr;
            if (rc > 0.0f && rc < INFINITY) {
                const V3 pc = v_scale(V3{ p.x, p.y, p.z }, rc / r);
                o = v_add(q_rot(rec.q, pc), rec.t);
            }
        }
        p.x = o.x; p.y = o.y; p.z = o.z;
        out[base + i] = p;
    }
}

// ---- Cartesian ----
struct SweepCartArgs {
    CartGrid C;
    PolarGrid G;
    int iterations;
};

// the value at azimuth coordinate u and measured range rho_m (rr_polar.h): 0 beyond the last bin, and where a corrected range is
// negative or not finite, which a pixel's own range never is
template <int INTERP>
__device__ inline uint8_t sweep_sample(const uint8_t* img, const PolarGrid& G, float u, float rho_m)
{
    if (!(rho_m >= 0.0f && rho_m < INFINITY)) return 0;
    float v;
    if (!range_coord(G, rho_m, &v)) return 0;
    return polar_sample<INTERP>(img, G, u, v);
}

// INTERP: 0 nearest, 1 bilinear (two kernels, so that traces and counters tell them apart).  Grid: (groups, frames)
template <int INTERP>
__global__ void __launch_bounds__(256) k_cartesian_sweep(const uint8_t* imgs, const float4* table, uint8_t* out, SweepCartArgs A)
{
    extern __shared__ __align__(16) float4 recs[];          // [n_angles][2]
    const size_t f = blockIdx.y;
    const float4* tab = table + 2 * f * (size_t)A.G.n_angles;
    for (int e = threadIdx.x; e < 2 * A.G.n_angles; e += blockDim.x) recs[e] = tab[e];
    __syncthreads();

    const uint32_t w = (uint32_t)A.C.width, wsq = w * w;
    const uint8_t* img = imgs + f * (size_t)A.G.n_cells * A.G.n_angles;
    uint8_t* o = out + f * wsq;
    for (uint32_t q = 4 * (blockIdx.x * blockDim.x + threadIdx.x); q < wsq; q += 4 * gridDim.x * blockDim.x) {
        uint32_t i = q / w, j = q - i * w;
        V3 P[4], Q[4];
        float u[4], dr[4];
        int a[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            // (pixels past the frame's last are computed at the next rows' places and dropped)
            P[e] = pixel_xy(A.C, i, j);
            Q[e] = P[e]; dr[e] = 0.0f;
            u[e] = az_coord(A.G, atan2f(P[e].y, P[e].x));
            a[e] = az_nearest(A.G, u[e]);
            if (++j == w) { j = 0; i++; }
        }
        for (int k = 0; k < A.iterations; k++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const SweepRec rec = rec_of(recs[2 * a[e]], recs[2 * a[e] + 1]);
                Q[e] = q_rot(q_conj(rec.q), v_sub(P[e], rec.t));
                dr[e] = rec.dr;
                u[e] = az_coord(A.G, atan2f(Q[e].y, Q[e].x));
                a[e] = az_nearest(A.G, u[e]);
            }
        }
        uint8_t v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float rho = sqrtf(v_dot(Q[e], Q[e]));
            v[e] = sweep_sample<INTERP>(img, A.G, u[e], rho + dr[e]);
        }
        if (q + 4 <= wsq && (reinterpret_cast<uintptr_t>(o + q) & 3) == 0) {
            *reinterpret_cast<uchar4*>(o + q) = make_uchar4(v[0], v[1], v[2], v[3]);
        } else {
            for (int e = 0; e < 4 && q + e < wsq; e++) o[q + e] = v[e];
        }
    }
}

}  // namespace

void launch_sweep_table(const float* az_poses, const float* ref_poses, const float* sensor_vel, float gain, int n_frames, const PolarGrid& G,
                        rr_sweep_rec* table, hipStream_t s)
{
    const size_t total = (size_t)n_frames * G.n_angles;
    const size_t groups = std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_sweep_table, dim3((unsigned)groups), dim3(256), 0, s, az_poses, ref_poses, sensor_vel, gain, G, total,
                       reinterpret_cast<float4*>(table));
}

void launch_compensate_points(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const rr_sweep_rec* table,
                              rr_radar_point* out, const PolarGrid& G, hipStream_t s)
{
    const dim3 grid((unsigned)std::min(1024, (max_points + 255) / 256), (unsigned)n_frames);
    hipLaunchKernelGGL(k_compensate_points, grid, dim3(256), 0, s, points, offsets, max_points, reinterpret_cast<const float4*>(table), out, G);
}

void launch_cartesian_sweep(const uint8_t* imgs, int n_frames, const rr_cartesian_config& cfg, const PolarGrid& G, const rr_sweep_rec* table,
                            int iterations, uint8_t* out, hipStream_t s)
{
    const SweepCartArgs A = { { cfg.width, cfg.pixel_size }, G, iterations };
    // a workgroup stages its frame's records once: as many workgroups per frame as fill the chip a few times over, no more
    const size_t wsq = (size_t)cfg.width * cfg.width;
    const size_t per_frame = std::max<size_t>(1, std::min<size_t>((wsq + 1023) / 1024, (4096 + n_frames - 1) / n_frames));
    const dim3 grid((unsigned)per_frame, (unsigned)n_frames);
    const size_t lds = (size_t)G.n_angles * sizeof(rr_sweep_rec);
    const float4* tab = reinterpret_cast<const float4*>(table);
    if (cfg.interpolation == 0) hipLaunchKernelGGL(k_cartesian_sweep<0>, grid, dim3(256), lds, s, imgs, tab, out, A);
    else hipLaunchKernelGGL(k_cartesian_sweep<1>, grid, dim3(256), lds, s, imgs, tab, out, A);
}

}  // namespace rr
