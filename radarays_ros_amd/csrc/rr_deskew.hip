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

#include <algorithm>

namespace rr {

namespace {

static_assert(sizeof(rr_sweep_rec) == 32, "a record is two float4");

struct SweepRec { Quat q; V3 t; float dr; };

__device__ inline SweepRec rec_of(float4 a, float4 b) { return { { a.x, a.y, a.z, a.w }, { b.x, b.y, b.z }, b.w }; }

// ---- the table ----
__global__ void __launch_bounds__(256) k_sweep_table(const float* az_poses, const float* ref_poses, const float* vel, float gain, int n_angles,
                                                     float theta_min, float theta_inc, size_t total, float4* table)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t f = e / (size_t)n_angles;
        const int a = (int)(e - f * (size_t)n_angles);
        const float* pa = az_poses + 7 * e;
        const float* pr = ref_poses + 7 * f;
        const Quat q_a = { pa[0], pa[1], pa[2], pa[3] }, q_ref = { pr[0], pr[1], pr[2], pr[3] };
        const V3 t_a = { pa[4], pa[5], pa[6] }, t_ref = { pr[4], pr[5], pr[6] };
        const Quat q = q_mul(q_conj(q_ref), q_a);
        const V3 t = q_rot(q_conj(q_ref), v_sub(t_a, t_ref));
        float dr = 0.0f;
        if (vel && gain != 0.0f) {
            const float theta = theta_min + (float)a * theta_inc;
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
                                                           rr_radar_point* out, int n_angles, int scroll, double resolution)
{
    const int f = blockIdx.y;
    const uint32_t total = offsets[(size_t)f * (n_angles + 1) + n_angles];
    const uint32_t m = min(total, (uint32_t)max_points);
    const size_t base = (size_t)f * max_points;
    const float4* tab = table + 2 * (size_t)f * n_angles;
    const float nan = __uint_as_float(0x7FC00000u);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        rr_radar_point p = points[base + i];
        V3 o = { nan, nan, nan };
        if (p.column < (uint32_t)n_angles) {                 // (a point that is not one of this shape has no azimuth)
            const int a = (int)p.column - scroll < 0 ? (int)p.column - scroll + n_angles : (int)p.column - scroll;
            const SweepRec rec = rec_of(tab[2 * a], tab[2 * a + 1]);
            const float r = (float)(((double)p.bin + 0.5) * resolution);
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
    int width;
    float pixel_size;
    int n_cells, n_angles, scroll;
    float theta_min, theta_inc, res;
    int iterations;
};

// the azimuth coordinate of a yaw: rr_detect.hip's cart_pixel, expression for expression; always in [0, n_angles)
__device__ inline float az_coord(float phi, const SweepCartArgs& A)
{
    const float na = (float)A.n_angles;
    float u = fmodf((phi - A.theta_min) / A.theta_inc, na);
    if (u < 0.0f) u += na;
    if (u >= na) u -= na;
    if (!(u >= 0.0f && u < na)) u = 0.0f;      // (a non-finite yaw, or a theta_inc so small that the quotient overflows)
    return u;
}

__device__ inline int az_nearest(float u, int n_angles)
{
    int a = (int)rintf(u);
    if (a >= n_angles) a -= n_angles;
    return a;
}

__device__ inline int sweep_z(const uint8_t* img, const SweepCartArgs& A, int b, int a)
{
    int col = a + A.scroll;
    if (col >= A.n_angles) col -= A.n_angles;
    return img[(size_t)b * A.n_angles + col];
}

// the value at (u, v): rr_detect.hip's cart_pixel from its range test on
template <int INTERP>
__device__ inline uint8_t sweep_sample(const uint8_t* img, const SweepCartArgs& A, float u, float rho_m)
{
    if (!(rho_m >= 0.0f && rho_m < INFINITY)) return 0;
    float v = rho_m / A.res - 0.5f;
    if (!(v <= (float)A.n_cells - 0.5f)) return 0;
    v = fmaxf(v, 0.0f);
    if (INTERP == 0) {
        const int a = az_nearest(u, A.n_angles);
        const int b = min((int)rintf(v), A.n_cells - 1);
        return (uint8_t)sweep_z(img, A, b, a);
    }
    const int a0 = min((int)floorf(u), A.n_angles - 1);
    const int a1 = a0 + 1 == A.n_angles ? 0 : a0 + 1;
    const float fu = u - (float)a0;
    const int b0 = (int)floorf(v), b1 = min(b0 + 1, A.n_cells - 1);
    const float fv = v - (float)b0;
    const int z00 = sweep_z(img, A, b0, a0), z01 = sweep_z(img, A, b0, a1), z10 = sweep_z(img, A, b1, a0), z11 = sweep_z(img, A, b1, a1);
    const float p0 = (1.0f - fu) * (float)z00 + fu * (float)z01;
    const float p1 = (1.0f - fu) * (float)z10 + fu * (float)z11;
    const float val = rintf((1.0f - fv) * p0 + fv * p1);
    return (uint8_t)fminf(fmaxf(val, 0.0f), 255.0f);
}

// INTERP: 0 nearest, 1 bilinear (two kernels, so that traces and counters tell them apart).  Grid: (groups, frames)
template <int INTERP>
__global__ void __launch_bounds__(256) k_cartesian_sweep(const uint8_t* imgs, const float4* table, uint8_t* out, SweepCartArgs A)
{
    extern __shared__ __align__(16) float4 recs[];          // [n_angles][2]
    const size_t f = blockIdx.y;
    const float4* tab = table + 2 * f * (size_t)A.n_angles;
    for (int e = threadIdx.x; e < 2 * A.n_angles; e += blockDim.x) recs[e] = tab[e];
    __syncthreads();

    const uint32_t w = (uint32_t)A.width, wsq = w * w;
    const uint8_t* img = imgs + f * (size_t)A.n_cells * A.n_angles;
    uint8_t* o = out + f * wsq;
    const float cc = (float)(A.width - 1) * 0.5f;
    for (uint32_t q = 4 * (blockIdx.x * blockDim.x + threadIdx.x); q < wsq; q += 4 * gridDim.x * blockDim.x) {
        uint32_t i = q / w, j = q - i * w;
        V3 P[4], Q[4];
        float u[4], dr[4];
        int a[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            // (pixels past the frame's last are computed at the next rows' places and dropped)
            P[e] = { (cc - (float)i) * A.pixel_size, (cc - (float)j) * A.pixel_size, 0.0f };
            Q[e] = P[e]; dr[e] = 0.0f;
            u[e] = az_coord(atan2f(P[e].y, P[e].x), A);
            a[e] = az_nearest(u[e], A.n_angles);
            if (++j == w) { j = 0; i++; }
        }
        for (int k = 0; k < A.iterations; k++) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const SweepRec rec = rec_of(recs[2 * a[e]], recs[2 * a[e] + 1]);
                Q[e] = q_rot(q_conj(rec.q), v_sub(P[e], rec.t));
                dr[e] = rec.dr;
                u[e] = az_coord(atan2f(Q[e].y, Q[e].x), A);
                a[e] = az_nearest(u[e], A.n_angles);
            }
        }
        uint8_t v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float rho = sqrtf(v_dot(Q[e], Q[e]));
            v[e] = sweep_sample<INTERP>(img, A, u[e], rho + dr[e]);
        }
        if (q + 4 <= wsq && (reinterpret_cast<uintptr_t>(o + q) & 3) == 0) {
            *reinterpret_cast<uchar4*>(o + q) = make_uchar4(v[0], v[1], v[2], v[3]);
        } else {
            for (int e = 0; e < 4 && q + e < wsq; e++) o[q + e] = v[e];
        }
    }
}

}  // namespace

void launch_sweep_table(const float* az_poses, const float* ref_poses, const float* sensor_vel, float gain, int n_frames, int n_angles,
                        float theta_min, float theta_inc, rr_sweep_rec* table, hipStream_t s)
{
    const size_t total = (size_t)n_frames * n_angles;
    const size_t groups = std::min<size_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(k_sweep_table, dim3((unsigned)groups), dim3(256), 0, s, az_poses, ref_poses, sensor_vel, gain, n_angles, theta_min, theta_inc,
                       total, reinterpret_cast<float4*>(table));
}

void launch_compensate_points(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const rr_sweep_rec* table,
                              rr_radar_point* out, int n_angles, int scroll, double resolution, hipStream_t s)
{
    const dim3 grid((unsigned)std::min(1024, (max_points + 255) / 256), (unsigned)n_frames);
    hipLaunchKernelGGL(k_compensate_points, grid, dim3(256), 0, s, points, offsets, max_points, reinterpret_cast<const float4*>(table), out, n_angles,
                       ((scroll % n_angles) + n_angles) % n_angles, resolution);
}

void launch_cartesian_sweep(const uint8_t* imgs, int n_frames, const rr_cartesian_config& cfg, int n_cells, int n_angles, int scroll, float theta_min,
                            float theta_inc, float res, const rr_sweep_rec* table, int iterations, uint8_t* out, hipStream_t s)
{
    SweepCartArgs A;
    A.width = cfg.width; A.pixel_size = cfg.pixel_size;
    A.n_cells = n_cells; A.n_angles = n_angles; A.scroll = ((scroll % n_angles) + n_angles) % n_angles;
    A.theta_min = theta_min; A.theta_inc = theta_inc; A.res = res;
    A.iterations = iterations;
    // a workgroup stages its frame's records once: as many workgroups per frame as fill the chip a few times over, no more
    const size_t wsq = (size_t)cfg.width * cfg.width;
    const size_t per_frame = std::max<size_t>(1, std::min<size_t>((wsq + 1023) / 1024, (4096 + n_frames - 1) / n_frames));
    const dim3 grid((unsigned)per_frame, (unsigned)n_frames);
    const size_t lds = (size_t)n_angles * sizeof(rr_sweep_rec);
    const float4* tab = reinterpret_cast<const float4*>(table);
    if (cfg.interpolation == 0) hipLaunchKernelGGL(k_cartesian_sweep<0>, grid, dim3(256), lds, s, imgs, tab, out, A);
    else hipLaunchKernelGGL(k_cartesian_sweep<1>, grid, dim3(256), lds, s, imgs, tab, out, A);
}

}  // namespace rr
