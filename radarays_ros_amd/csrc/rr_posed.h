// rr_posed.h -- the posed scene, stated once for the refit kernels and the mesh slicer (rr_refit.hip, rr_slice.hip): every face's rest corners
// moved by its object's rigid pose [7] = qx qy qz qw tx ty tz.  All f32, nothing fused.
#pragma once
#include "rr_device.h"

namespace rr {

// p' = q_rot(q, p) + t in f32, un-fused (the files are compiled with -ffp-contract=off); the exact identity
// (0,0,0,1,0,0,0) is a plain copy, so the sign of a zero coordinate never changes
__device__ inline bool pose_is_identity(const float* P)
{
    return P[0] == 0.0f && P[1] == 0.0f && P[2] == 0.0f && P[3] == 1.0f && P[4] == 0.0f && P[5] == 0.0f && P[6] == 0.0f;
}
__device__ inline V3 pose_point(const float* P, bool ident, V3 p)
{
    if (ident) return p;
    const Quat q = { P[0], P[1], P[2], P[3] };
    const V3 r = q_rot(q, p);
    return { r.x + P[4], r.y + P[5], r.z + P[6] };
}
__device__ inline V3 ld_vert(const float* verts, uint32_t i)
{
    const float* v = verts + 3 * (size_t)i;
    return { v[0], v[1], v[2] };
}
// the three posed corners (a, b, c) of face f under the pose of `object`
__device__ inline void posed_face(const float* verts, const uint32_t* faces, const float* poses, uint32_t f, uint32_t object,
                                  V3& a, V3& b, V3& c)
{
    const float* P = poses + 7 * (size_t)object;
    const bool ident = pose_is_identity(P);
    const uint32_t* fv = faces + 3 * (size_t)f;
    a = pose_point(P, ident, ld_vert(verts, fv[0]));
    b = pose_point(P, ident, ld_vert(verts, fv[1]));
    c = pose_point(P, ident, ld_vert(verts, fv[2]));
}

}  // namespace rr
