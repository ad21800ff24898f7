// rr_pose2d.h -- the rigid 2-D state (c, s, tx, ty) and the ICP step, stated once for the scan matcher, the likelihood field, occupancy
// mapping, the particle filter, map refinement and the beam model (rr_icp.hip, rr_field.hip, rr_occupancy.hip, rr_filter.hip, rr_refine.hip,
// rr_cast.hip).  A state moves a point (x, y) to px = (c * x - s * y) + tx, py = (s * x + c * y) + ty: the parentheses are part of the
// definition.  Kernels apply a state in f32; a state kept in f64 is rounded to f32 first.  All f32 but the solve, nothing fused.
#pragma once
#include "../../include/radarays_mi355.h"
#include <hip/hip_runtime.h>

namespace rr {

struct Pose2 { float c, s, tx, ty; };

__device__ inline Pose2 pose_round(double c, double s, double tx, double ty) { return { (float)c, (float)s, (float)tx, (float)ty }; }
// state f of an f64 table rounded to f32; a null table: the identity
__device__ inline Pose2 pose_of(const double* states, size_t f)
{
    if (!states) return { 1.0f, 0.0f, 0.0f, 0.0f };
    return pose_round(states[4 * f], states[4 * f + 1], states[4 * f + 2], states[4 * f + 3]);
}
__device__ inline Pose2 pose_of(const float* states, size_t h) { return { states[4 * h], states[4 * h + 1], states[4 * h + 2], states[4 * h + 3] }; }

__device__ inline void pose_move(const Pose2& p, float x, float y, float* px, float* py)
{
    *px = (p.c * x - p.s * y) + p.tx;
    *py = (p.s * x + p.c * y) + p.ty;
}
// a map-frame point back into the state's own frame (the inverse sensor model's direction)
__device__ inline void pose_unmove(const Pose2& p, float qx, float qy, float* px, float* py)
{
    const float dx = qx - p.tx, dy = qy - p.ty;
    *px = p.c * dx + p.s * dy;
    *py = p.c * dy - p.s * dx;
}

// the point count of frame f of a detected batch, cut at max_points; *truncated (may be null): it was cut
__device__ inline uint32_t frame_count(const uint32_t* offsets, int f, int n_angles, int max_points, bool* truncated)
{
    const uint32_t total = offsets[(size_t)f * (n_angles + 1) + n_angles];
    if (truncated) *truncated = total > (uint32_t)max_points;
    return min(total, (uint32_t)max_points);
}

// ---- the ICP step of the header (rr_register_points, rr_refine_poses): the eight sums over the matched pairs, and the closed-form solve ----
enum { S_N = 0, S_PX, S_PY, S_QX, S_QY, S_DOT, S_CROSS, S_SSE, S_COUNT };
struct Pose2d { double c, s, tx, ty; };                          // a state between solves.  `State` below: this, or an rr_icp_rec

// the start: (c, s) normalised once; true for a state with no direction, which becomes the identity (the caller flags RR_ICP_DEGENERATE)
template <class State> __device__ inline bool icp_start(State& st)
{
    const double h = sqrt(st.c * st.c + st.s * st.s);
    const bool directed = h > 0.0 && h < (double)INFINITY;
    if (directed) { st.c = st.c / h; st.s = st.s / h; }
    else { st.c = 1.0; st.s = 0.0; st.tx = 0.0; st.ty = 0.0; }
    return !directed;
}

// one matched pair, moved point p and target q, quantised to 1/256 m and added to the eight sums.
// Exact because |P|, |Q| <= 2^21: the matcher matches only coordinates below PointResidual::kRange = 8192 in magnitude, refinement only points IN GRID and
// cell centres of a grid that its check holds within +-8192 m.  So P - Q fits 32 bits and every product 32 x 32 -> 64; the sums are integers
__device__ inline void icp_accumulate(long long* sum, float px, float py, float qx, float qy)
{
    const int32_t Px = (int32_t)rintf(px * 256.0f), Py = (int32_t)rintf(py * 256.0f);
    const int32_t Qx = (int32_t)rintf(qx * 256.0f), Qy = (int32_t)rintf(qy * 256.0f);
    const int32_t ex = Px - Qx, ey = Py - Qy;
    sum[S_N] += 1;
    sum[S_PX] += Px; sum[S_PY] += Py; sum[S_QX] += Qx; sum[S_QY] += Qy;
    sum[S_DOT] += (long long)Px * Qx + (long long)Py * Qy;
    sum[S_CROSS] += (long long)Px * Qy - (long long)Py * Qx;
    sum[S_SSE] += (long long)ex * ex + (long long)ey * ey;
}

// the SOLVE: f64, + - * / sqrt only, evaluated as written.  True for a degenerate step (fewer than 2 pairs, or no direction): the state is kept
template <class State> __device__ inline bool icp_solve(const long long* S, State& st)
{
    const double N = (double)S[S_N], SPx = (double)S[S_PX], SPy = (double)S[S_PY], SQx = (double)S[S_QX], SQy = (double)S[S_QY];
    const double Sdot = (double)S[S_DOT], Scross = (double)S[S_CROSS];
    const double A = N * Sdot - (SPx * SQx + SPy * SQy);
    const double B = N * Scross - (SPx * SQy - SPy * SQx);
    const double h = sqrt(A * A + B * B);
    if (S[S_N] < 2 || !(h > 0.0)) return true;
    const double c = st.c, s = st.s, tx = st.tx, ty = st.ty;
    const double dc = A / h, ds = B / h;
    const double mpx = (SPx / N) / 256.0, mpy = (SPy / N) / 256.0, mqx = (SQx / N) / 256.0, mqy = (SQy / N) / 256.0;
    const double dtx = mqx - (dc * mpx - ds * mpy);
    const double dty = mqy - (ds * mpx + dc * mpy);
    const double c1 = dc * c - ds * s;
    const double s1 = ds * c + dc * s;
    const double tx1 = (dc * tx - ds * ty) + dtx;
    const double ty1 = (ds * tx + dc * ty) + dty;
    const double nrm = sqrt(c1 * c1 + s1 * s1);
    st.c = c1 / nrm; st.s = s1 / nrm; st.tx = tx1; st.ty = ty1;
    return false;
}

// The residuals of the matcher (rr_icp.hip).  A residual names its target record, its sums and its coordinate range, and gives: stage(), the
// (x, y) of target j for the LDS tile, or (+inf, +inf) if it may not be a candidate; accumulate(), which fetches what it needs of the matched
// target; solve() and sse().  Point-to-point: x and y lead a 24-byte point, the step above
struct PointResidual {
    using Target = rr_radar_point;
    enum { COUNT = S_COUNT, N = S_N };
    static constexpr float kRange = 8192.0f;                     // a coordinate must be finite and below this in magnitude (icp_accumulate relies on it)
    static __device__ inline bool in_range(float v) { return fabsf(v) < kRange; }      // false for NaN and infinities
    static __device__ inline float2 stage(const Target* tgt, uint32_t j, bool live)
    {
        float x = INFINITY, y = INFINITY;
        if (live) {
            const float qx = tgt[j].x, qy = tgt[j].y;
            if (in_range(qx) && in_range(qy)) { x = qx; y = qy; }
        }
        return make_float2(x, y);
    }
    static __device__ inline void accumulate(long long* sum, float px, float py, const Target* tgt, uint32_t j) { icp_accumulate(sum, px, py, tgt[j].x, tgt[j].y); }
    template <class State> static __device__ inline bool solve(const long long* S, State& st) { return icp_solve(S, st); }
    static __device__ inline long long sse(const long long* S) { return S[S_SSE]; }
};

// ---- the point-to-line step of the header (rr_register_surfels): the fourteen sums over the matched pairs, and the LDL^T solve ----
enum { L_N = 0, L_H00LO, L_H00HI, L_H01, L_H02, L_H11, L_H12, L_H22, L_G0LO, L_G0HI, L_G1, L_G2, L_RRLO, L_RRHI, L_COUNT };

// a term that may pass 2^63 over 65,536 pairs, split before any reduction: lo in 0 .. 2^32-1, hi the arithmetic shift
__device__ inline void line_limbs(long long* sum, int lo, long long t)
{
    sum[lo] += t & 0xFFFFFFFFll;
    sum[lo + 1] += t >> 32;
}
__device__ inline double line_join(const long long* S, int lo) { return (double)S[lo + 1] * 4294967296.0 + (double)S[lo]; }

// one matched pair: moved point p and surfel mean q quantised to 1/64 m, the surfel's normal to 1/1024.  Exact because the matcher matches
// only coordinates below LineResidual::kRange = 2048 and normal components of at most 1 in magnitude: |P|, |Q| <= 2^17, |M| <= 2^10, so |r| <= 2^29,
// |a0| <= 2^28, and every term is below 2^58 (the header lists each term's and each sum's bound)
__device__ inline void line_accumulate(long long* sum, float px, float py, float qx, float qy, float nx, float ny)
{
    const int32_t Px = (int32_t)rintf(px * 64.0f), Py = (int32_t)rintf(py * 64.0f);
    const int32_t Qx = (int32_t)rintf(qx * 64.0f), Qy = (int32_t)rintf(qy * 64.0f);
    const long long Mx = (int32_t)rintf(nx * 1024.0f), My = (int32_t)rintf(ny * 1024.0f);
    const long long ex = Px - Qx, ey = Py - Qy;
    const long long r = Mx * ex + My * ey;
    const long long a0 = (long long)Px * My - (long long)Py * Mx;
    sum[L_N] += 1;
    line_limbs(sum, L_H00LO, a0 * a0);
    sum[L_H01] += a0 * Mx; sum[L_H02] += a0 * My;
    sum[L_H11] += Mx * Mx; sum[L_H12] += Mx * My; sum[L_H22] += My * My;
    line_limbs(sum, L_G0LO, a0 * r);
    sum[L_G1] += Mx * r; sum[L_G2] += My * r;
    line_limbs(sum, L_RRLO, r * r);
}

// sse of the record: rrhi * 2^32 + rrlo in (1/65536 m)^2, saturated
__device__ inline long long line_sse(const long long* S)
{
    return S[L_RRHI] >= (1ll << 30) ? 0x7FFFFFFFFFFFFFFFll : S[L_RRHI] * 4294967296ll + S[L_RRLO];
}

// the SOLVE: H delta = -g by an explicit LDL^T, f64, + - * / and the renormalisation's sqrt, evaluated as written.  True for a degenerate
// step (fewer than 3 pairs, or a pivot that is not > 0): the state is kept
template <class State> __device__ inline bool line_solve(const long long* S, State& st)
{
    if (S[L_N] < 3) return true;
    const double H00 = line_join(S, L_H00LO), H01 = (double)S[L_H01], H02 = (double)S[L_H02];
    const double H11 = (double)S[L_H11], H12 = (double)S[L_H12], H22 = (double)S[L_H22];
    const double g0 = line_join(S, L_G0LO), g1 = (double)S[L_G1], g2 = (double)S[L_G2];
    const double d0 = H00;
    if (!(d0 > 0.0)) return true;
    const double l10 = H01 / d0, l20 = H02 / d0;
    const double d1 = H11 - l10 * H01;
    if (!(d1 > 0.0)) return true;
    const double m21 = H12 - l20 * H01;
    const double l21 = m21 / d1;
    const double d2 = (H22 - l20 * H02) - l21 * m21;
    if (!(d2 > 0.0)) return true;
    const double z0 = -g0;
    const double z1 = -g1 - l10 * z0;
    const double z2 = (-g2 - l20 * z0) - l21 * z1;
    const double x2 = z2 / d2;
    const double x1 = z1 / d1 - l21 * x2;
    const double x0 = (z0 / d0 - l10 * x1) - l20 * x2;
    const double u = x0 / 2.0;
    const double dc = (1.0 - u * u) / (1.0 + u * u), ds = (2.0 * u) / (1.0 + u * u);
    const double dtx = x1 / 64.0, dty = x2 / 64.0;
    const double c = st.c, s = st.s, tx = st.tx, ty = st.ty;
    const double c1 = dc * c - ds * s;
    const double s1 = ds * c + dc * s;
    const double tx1 = (dc * tx - ds * ty) + dtx;
    const double ty1 = (ds * tx + dc * ty) + dty;
    const double nrm = sqrt(c1 * c1 + s1 * s1);
    st.c = c1 / nrm; st.s = s1 / nrm; st.tx = tx1; st.ty = ty1;
    return false;
}

// point-to-line: (x, y, nx, ny) leads a 32-byte surfel and is one 16-byte load; a normal component above 1 in magnitude (or NaN) is no candidate
struct LineResidual {
    using Target = rr_surfel;
    enum { COUNT = L_COUNT, N = L_N };
    static constexpr float kRange = 2048.0f;                     // a coordinate must be finite and below this in magnitude (line_accumulate relies on it)
    static __device__ inline float4 lead(const Target* tgt, uint32_t j) { return reinterpret_cast<const float4*>(tgt)[2 * (size_t)j]; }
    static __device__ inline bool in_range(float v) { return fabsf(v) < kRange; }
    static __device__ inline float2 stage(const Target* tgt, uint32_t j, bool live)
    {
        float x = INFINITY, y = INFINITY;
        if (live) {
            const float4 q = lead(tgt, j);
            if (in_range(q.x) && in_range(q.y) && fabsf(q.z) <= 1.0f && fabsf(q.w) <= 1.0f) { x = q.x; y = q.y; }
        }
        return make_float2(x, y);
    }
    static __device__ inline void accumulate(long long* sum, float px, float py, const Target* tgt, uint32_t j)
    {
        const float4 q = lead(tgt, j);                               // the normal is fetched once, here
        line_accumulate(sum, px, py, q.x, q.y, q.z, q.w);
    }
    template <class State> static __device__ inline bool solve(const long long* S, State& st) { return line_solve(S, st); }
    static __device__ inline long long sse(const long long* S) { return line_sse(S); }
};

// ---- the block preconditioner of the header (rr_optimize_graph): line_solve's LDL^T kept as factors, for a block with H12 = 0 ----
struct Ldl3 { double l10, l20, l21, d0, d1, d2; };

// the factors of [ H00 H01 H02 ; H01 H11 0 ; H02 0 H22 ]; false for a pivot that is not > 0 (tested as each is formed)
__device__ inline bool ldl3_factor(double H00, double H01, double H02, double H11, double H22, Ldl3& f)
{
    f.d0 = H00;
    if (!(f.d0 > 0.0)) return false;
    f.l10 = H01 / f.d0; f.l20 = H02 / f.d0;
    f.d1 = H11 - f.l10 * H01;
    if (!(f.d1 > 0.0)) return false;
    const double m21 = 0.0 - f.l20 * H01;
    f.l21 = m21 / f.d1;
    f.d2 = (H22 - f.l20 * H02) - f.l21 * m21;
    return f.d2 > 0.0;
}

// x = (L D L^T)^-1 v
__device__ inline void ldl3_solve(const Ldl3& f, const double* v, double* x)
{
    const double z0 = v[0];
    const double z1 = v[1] - f.l10 * z0;
    const double z2 = (v[2] - f.l20 * z0) - f.l21 * z1;
    x[2] = z2 / f.d2;
    x[1] = z1 / f.d1 - f.l21 * x[2];
    x[0] = (z0 / f.d0 - f.l10 * x[1]) - f.l20 * x[2];
}

}  // namespace rr
