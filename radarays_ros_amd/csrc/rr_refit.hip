// rr_refit.hip -- gfx950 kernels of dynamic scenes: per-object rigid poses applied to the rest geometry, and the tree's
// boxes recomputed in place for the moved triangles (rr_set_object_poses / rr_update_vertices / rr_rebuild_tree).
//
// The tree keeps its topology: every TriRec keeps its face and object id, every child record its reference and the parent
// link in node record 0's spare word.  What changes is the triangle data (v0, e1, e2 and the grazing threshold) and the
// lo / hi of every child record.  The nearest hit does not depend on the tree (the grazing guard makes it a property of the
// mesh and hit_pad), so a refit tree renders what a fresh build of the posed triangle soup renders.
//
//   k_refit_extent  min / max of the posed corners + a non-finite flag, per workgroup (the host finishes it: it validates
//                   the call before the first write and forms hit_pad and the box padding from it)
//   k_refit_tris    one thread per TriRec: posed corners -> v0, e1 = b - a, e2 = c - a, grazing threshold
//   k_refit_level   one launch per tree level, deepest first, one quad per node: lane q recomputes child q's box
//   k_tree_cost     half-area sum over all child records, per workgroup
//   k_gather_refs   the child references, for the host's per-level node lists
//   k_pose_soup     the posed triangle soup (face order) for a rebuild
//
// Kernel boundaries order the levels: a level reads only boxes the previous launch wrote, so no workgroup waits for
// another and no cross-XCD fence is needed inside a launch.  No kernel here uses scratch (tests/test_dynamic_host.py).
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_posed.h"

namespace rr {

namespace {

constexpr int kRefitTB = 256;

// (the posed corners of a face, posed_face: rr_posed.h)
__device__ inline void grow(float lo[3], float hi[3], V3 p)
{
    lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
    hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
}
__device__ inline bool finite3(V3 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// out[blockIdx.x][8] = lo xyz, hi xyz, non-finite flag (0 / 1), 0.  Every face has at least one record (the builders
// never drop a reference), so the records' faces are all faces: the result is the min / max guard_pad forms on the soup.
__global__ void __launch_bounds__(kRefitTB) k_refit_extent(const TriRec* tris, size_t n, const float* verts,
                                                           const uint32_t* faces, const float* poses, float* out)
{
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    float bad = 0.0f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        V3 a, b, c;
        posed_face(verts, faces, poses, tris[i].face, tris[i].object, a, b, c);
        if (!(finite3(a) && finite3(b) && finite3(c))) bad = 1.0f;
        grow(lo, hi, a); grow(lo, hi, b); grow(lo, hi, c);
    }
    __shared__ float red[7][kRefitTB];
    for (int k = 0; k < 3; k++) { red[k][threadIdx.x] = lo[k]; red[3 + k][threadIdx.x] = hi[k]; }
    red[6][threadIdx.x] = bad;
    __syncthreads();
    for (int s = kRefitTB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            for (int k = 0; k < 3; k++) {
                red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + s]);
                red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + s]);
            }
            red[6][threadIdx.x] = fmaxf(red[6][threadIdx.x], red[6][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 8) out[(size_t)blockIdx.x * 8 + threadIdx.x] = threadIdx.x < 7 ? red[threadIdx.x][0] : 0.0f;
}

// v0 = a, e1 = b - a, e2 = c - a (the builders' f32 ops, rr_bvh.cpp emit_leaf), the grazing threshold as k_tri_graze
// forms it; face and object stay
__global__ void __launch_bounds__(kRefitTB) k_refit_tris(TriRec* tris, size_t n, const float* verts, const uint32_t* faces,
                                                         const float* poses)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    TriRec& r = tris[i];
    V3 a, b, c;
    posed_face(verts, faces, poses, r.face, r.object, a, b, c);
    const V3 e1 = v_sub(b, a), e2 = v_sub(c, a);
    const V3 x = v_cross(e1, e2);
    r.v0[0] = a.x; r.v0[1] = a.y; r.v0[2] = a.z;
    r.e1[0] = e1.x; r.e1[1] = e1.y; r.e1[2] = e1.z;
    r.e2[0] = e2.x; r.e2[1] = e2.y; r.e2[2] = e2.z;
    r.pad = __float_as_uint(2.5e-5f * v_dot(x, x));
}

// One level of the tree: level_nodes[0..n) are node indices, lane q of quad k recomputes child q of node level_nodes[k].
// A leaf child's box is the union of its records' corners as traversal forms them (v0, v0 + e1, v0 + e2) padded by
// `inflate`; an inner child's box is the union of its node's non-empty child boxes (written by the previous launch), which
// already carry the padding.  Only lo / hi are written: the reference and the spare word (parent link) stay.
// Records of objects that have not moved since the tree was built (moved[object] == 0: the same pose, the same rest
// vertices) keep what the builder knew: a spatial split files a part of a large face into each of several leaves, and the
// leaf's as-built box (`built`, a copy of the nodes taken before the first refit) bounds only that part -- the whole
// triangle's box would stretch every such leaf over the face (a 420 m floor over hundreds of leaves).  Such a record's box
// is its triangle's box clipped to the as-built leaf box; a leaf of static records only keeps its as-built box, widened
// by `extra` when the scene's extent (and with it the padding rule) has grown since the build.
__global__ void __launch_bounds__(kRefitTB) k_refit_level(float4* base4, const uint32_t* level_nodes, size_t n_nodes,
                                                          float inflate, const float4* built4, const uint8_t* moved, float extra)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 4 * n_nodes) return;
    Node4* nodes = reinterpret_cast<Node4*>(base4);
    Child4& ch = nodes[level_nodes[t >> 2]].c[t & 3];
    const uint32_t ref = ch.ref;
    if (ref == kEmptyRef) return;
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    if (ref & kLeafFlag) {
        const uint32_t first = ref & 0x0FFFFFFFu, cnt = ((ref >> 28) & 7u) + 1u;
        const Child4& bc = reinterpret_cast<const Node4*>(built4)[level_nodes[t >> 2]].c[t & 3];
        bool all_static = true;
        for (uint32_t k = 0; k < cnt; k++) {
            const TriRec& r = *reinterpret_cast<const TriRec*>(base4 + first + 3u * k);
            const V3 v0 = { r.v0[0], r.v0[1], r.v0[2] };
            float tl[3] = { INFINITY, INFINITY, INFINITY }, th[3] = { -INFINITY, -INFINITY, -INFINITY };
            grow(tl, th, v0);
            grow(tl, th, v_add(v0, { r.e1[0], r.e1[1], r.e1[2] }));
            grow(tl, th, v_add(v0, { r.e2[0], r.e2[1], r.e2[2] }));
            if (!moved[r.object]) {
                float cl[3], chh[3];
                bool ok = true;
                for (int a = 0; a < 3; a++) {
                    cl[a] = fmaxf(tl[a], bc.lo[a]); chh[a] = fminf(th[a], bc.hi[a]);
                    ok = ok && cl[a] <= chh[a];
                }
                if (ok) for (int a = 0; a < 3; a++) { tl[a] = cl[a]; th[a] = chh[a]; }
            } else {
                all_static = false;
            }
            for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], tl[a]); hi[a] = fmaxf(hi[a], th[a]); }
        }
        if (all_static) {
            for (int k = 0; k < 3; k++) { lo[k] = bc.lo[k] - extra; hi[k] = bc.hi[k] + extra; }
        } else {
            for (int k = 0; k < 3; k++) { lo[k] = lo[k] - inflate; hi[k] = hi[k] + inflate; }
        }
    } else {
        const Node4& cn = nodes[ref >> 3];
        for (int q = 0; q < 4; q++) {
            if (cn.c[q].ref == kEmptyRef) continue;
            for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], cn.c[q].lo[k]); hi[k] = fmaxf(hi[k], cn.c[q].hi[k]); }
        }
    }
    for (int k = 0; k < 3; k++) { ch.lo[k] = lo[k]; ch.hi[k] = hi[k]; }
}

// out[blockIdx.x] = sum over this workgroup's child records of half-area x (1 for an inner child, count for a leaf child)
__global__ void __launch_bounds__(kRefitTB) k_tree_cost(const Node4* nodes, size_t n_children, double* out)
{
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_children; i += (size_t)gridDim.x * blockDim.x) {
        const Child4& ch = nodes[i >> 2].c[i & 3];
        if (ch.ref == kEmptyRef) continue;
        const double dx = (double)ch.hi[0] - ch.lo[0], dy = (double)ch.hi[1] - ch.lo[1], dz = (double)ch.hi[2] - ch.lo[2];
        const double w = (ch.ref & kLeafFlag) ? (double)(((ch.ref >> 28) & 7u) + 1u) : 1.0;
        acc += w * (dx * dy + dy * dz + dz * dx);
    }
    __shared__ double red[kRefitTB];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kRefitTB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(kRefitTB) k_gather_refs(const Node4* nodes, size_t n_children, uint32_t* out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_children) out[i] = nodes[i >> 2].c[i & 3].ref;
}

// soup[face] = the face's three posed corners, obj[face] = its object id (a face cut by spatial splits has several records:
// they write the same values)
__global__ void __launch_bounds__(kRefitTB) k_pose_soup(const TriRec* tris, size_t n, const float* verts, const uint32_t* faces,
                                                        const float* poses, float* soup, uint32_t* obj)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = tris[i].face, o = tris[i].object;
    V3 a, b, c;
    posed_face(verts, faces, poses, f, o, a, b, c);
    float* s = soup + 9 * (size_t)f;
    s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = b.x; s[4] = b.y; s[5] = b.z; s[6] = c.x; s[7] = c.y; s[8] = c.z;
    obj[f] = o;
}

inline unsigned grid_for(size_t n) { return (unsigned)((n + kRefitTB - 1) / kRefitTB); }

}  // namespace

// ---------------------------------------------------------------------------
// launchers (declared in rr_launch.h, called from rr_scene.hip)
// ---------------------------------------------------------------------------
constexpr int kRefitReduceGroups = 1024;    // workgroups of the two reductions (fixed: the sums are formed in a fixed order)
int refit_reduce_groups() { return kRefitReduceGroups; }

void launch_refit_extent(const TriRec* tris, size_t n, const float* verts, const uint32_t* faces, const float* poses,
                         float* out8, hipStream_t s)
{
    hipLaunchKernelGGL(k_refit_extent, dim3(kRefitReduceGroups), dim3(kRefitTB), 0, s, tris, n, verts, faces, poses, out8);
}
void launch_refit_tris(TriRec* tris, size_t n, const float* verts, const uint32_t* faces, const float* poses, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_refit_tris, dim3(grid_for(n)), dim3(kRefitTB), 0, s, tris, n, verts, faces, poses);
}
// levels: node indices grouped by depth, level d = [level_off[d], level_off[d + 1]); deepest level first
void launch_refit_levels(float4* base4, const uint32_t* level_nodes, const uint32_t* level_off, int n_levels, float inflate,
                         const float4* built4, const uint8_t* moved, float extra, hipStream_t s)
{
    for (int d = n_levels - 1; d >= 0; d--) {
        const size_t n = (size_t)level_off[d + 1] - level_off[d];
        if (n) hipLaunchKernelGGL(k_refit_level, dim3(grid_for(4 * n)), dim3(kRefitTB), 0, s, base4, level_nodes + level_off[d], n, inflate,
                                  built4, moved, extra);
    }
}
void launch_tree_cost(const Node4* nodes, size_t n_nodes, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_tree_cost, dim3(kRefitReduceGroups), dim3(kRefitTB), 0, s, nodes, 4 * n_nodes, out);
}
void launch_gather_refs(const Node4* nodes, size_t n_nodes, uint32_t* out, hipStream_t s)
{
    if (n_nodes) hipLaunchKernelGGL(k_gather_refs, dim3(grid_for(4 * n_nodes)), dim3(kRefitTB), 0, s, nodes, 4 * n_nodes, out);
}
void launch_pose_soup(const TriRec* tris, size_t n, const float* verts, const uint32_t* faces, const float* poses,
                      float* soup, uint32_t* obj, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_pose_soup, dim3(grid_for(n)), dim3(kRefitTB), 0, s, tris, n, verts, faces, poses, soup, obj);
}

}  // namespace rr
