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
// Exact because |P|, |Q| <= 2^21: the matcher matches only coordinates below kIcpRange = 8192 in magnitude, refinement only points IN GRID and
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

}  // namespace rr
