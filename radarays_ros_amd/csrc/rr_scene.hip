// rr_scene.hip -- the scene of a context: mesh upload (host SAH tree with the measured tree choice, GPU LBVH, a copy of another context's
// tree), dynamic scenes (poses and new rest vertices refit in place, rr_refit.hip; tree cost and rebuild) and rr_get_bvh_info.
#include "rr_ctx.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>

namespace {

// child references are 28-bit float4 offsets from the base of the tree allocation (rr_bvh.h)
int check_bvh_size(rr_ctx* c, size_t n_nodes, size_t n_tris)
{
    if (n_nodes * 8 + (n_tris + 4) * 3 >= (1ull << 28))
        return fail(c, -4, "rr_set_mesh: tree too large for 28-bit references (8 x nodes + 3 x triangles must stay below 2^28: about 60M triangles)");
    return 0;
}

// The grazing guard's padding (leaf_step, rr_kernels.hip): 1e-5 x max(extent, largest |coordinate|) of the vertices the faces
// use -- half of what both builders pad their boxes with (2e-5 x the same measure + 1e-6; the GPU builder measures ALL
// vertices, which can only give more).  One multiplication: nothing a compiler could contract; the oracle forms the same value
float guard_pad(const float* verts, const uint32_t* faces, size_t nf)
{
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (size_t i = 0; i < 3 * nf; i++) {
        const float* v = verts + 3 * (size_t)faces[i];
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], v[k]); hi[k] = std::max(hi[k], v[k]); }
    }
    if (nf == 0) return 0.f;
    float ext = 0.f, mag = 0.f;
    for (int k = 0; k < 3; k++) { ext = std::max(ext, hi[k] - lo[k]); mag = std::max(mag, std::max(std::fabs(lo[k]), std::fabs(hi[k]))); }
    return 1e-5f * std::max(ext, mag);
}

// ---- dynamic scenes -------------------------------------------------------------------------------------------------
// rr_set_mesh* keeps a device copy of the rest geometry (12 B per vertex + 12 B per face; object ids ride in the triangle
// records) and resets every object's pose to the identity
int keep_rest(rr_ctx* c, const float* verts, size_t nv, const uint32_t* faces, size_t nf, const uint32_t* face_object_id)
{
    c->dyn_ready = false; c->cost_known = false; c->have_built = false; c->verts_dirty = false;
    if (c->rebuilding) { c->build_poses = c->poses; return 0; }     // rr_rebuild_tree keeps the rest data it had
    uint32_t n_obj = 1;
    if (face_object_id) for (size_t f = 0; f < nf; f++) n_obj = std::max(n_obj, face_object_id[f] + 1u);
    RR_HIP(c, c->d_rest_v.ensure(3 * nv));
    RR_HIP(c, c->d_rest_f.ensure(3 * nf));
    if (nv) RR_HIP(c, hipMemcpy(c->d_rest_v.p, verts, 3 * nv * sizeof(float), hipMemcpyHostToDevice));
    if (nf) RR_HIP(c, hipMemcpy(c->d_rest_f.p, faces, 3 * nf * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->rest_nv = nv; c->rest_nf = nf; c->n_objects = n_obj;
    c->poses.assign(7 * (size_t)n_obj, 0.0f);
    for (uint32_t o = 0; o < n_obj; o++) c->poses[7 * (size_t)o + 3] = 1.0f;
    c->build_poses = c->poses;
    c->twists.assign(6 * (size_t)n_obj, 0.0f);
    RR_HIP(c, c->d_poses.ensure(c->poses.size()));
    RR_HIP(c, hipMemcpy(c->d_poses.p, c->poses.data(), c->poses.size() * sizeof(float), hipMemcpyHostToDevice));
    c->d_stage_v.release(); c->d_stage_poses.release();
    return 0;
}

TriRec* dev_tris(rr_ctx* c) { return reinterpret_cast<TriRec*>(c->d_bvh.p + c->tri_base4); }

// SAH-style cost of the current boxes: sum over child records of half-area / the root's half-area, weighted 1 per inner
// child and `count` per leaf child (the per-workgroup partials are summed here in a fixed order: the same boxes give the
// same value)
int tree_cost(rr_ctx* c, double* cost)
{
    const int G = refit_reduce_groups();
    RR_HIP(c, c->d_cost.ensure((size_t)G));
    launch_tree_cost(reinterpret_cast<const Node4*>(c->d_bvh.p), c->n_nodes, c->d_cost.p, c->stream);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<double> part((size_t)G);
    RR_HIP(c, hipMemcpy(part.data(), c->d_cost.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    Node4 root;
    RR_HIP(c, hipMemcpy(&root, c->d_bvh.p, sizeof(Node4), hipMemcpyDeviceToHost));
    double sum = 0.0;
    for (double x : part) sum += x;
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    for (int q = 0; q < 4; q++) {
        if (root.c[q].ref == kEmptyRef) continue;
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], (double)root.c[q].lo[k]); hi[k] = std::max(hi[k], (double)root.c[q].hi[k]); }
    }
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    const double ha = (dx > 0.0 || dy > 0.0 || dz > 0.0) ? dx * dy + dy * dz + dz * dx : 0.0;
    *cost = ha > 0.0 ? sum / ha : 0.0;
    return 0;
}

// once per tree, at its first dynamic call: the per-level node lists (frontier expansion from the root over the child
// references) and the cost of the boxes as built
int refit_prepare(rr_ctx* c)
{
    if (c->dyn_ready) return 0;
    const size_t nn = c->n_nodes;
    std::vector<uint32_t> refs(4 * nn);
    if (nn) {
        DevBuf<uint32_t> d_refs;
        RR_HIP(c, d_refs.ensure(4 * nn));
        launch_gather_refs(reinterpret_cast<const Node4*>(c->d_bvh.p), nn, d_refs.p, c->stream);
        RR_HIP(c, hipGetLastError());
        RR_HIP(c, hipStreamSynchronize(c->stream));
        RR_HIP(c, hipMemcpy(refs.data(), d_refs.p, refs.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    std::vector<uint32_t> order;
    order.reserve(nn);
    c->level_off.assign(1, 0u);
    if (nn) order.push_back(0u);
    for (size_t b = 0; b < order.size();) {
        const size_t e = order.size();
        for (size_t i = b; i < e; i++)
            for (int q = 0; q < 4; q++) {
                const uint32_t r = refs[4 * (size_t)order[i] + q];
                if (r == kEmptyRef || (r & kLeafFlag)) continue;
                if ((r >> 3) >= nn || order.size() >= nn) return fail(c, -4, "dynamic scene: the tree's references are inconsistent");
                order.push_back(r >> 3);
            }
        c->level_off.push_back((uint32_t)e);
        b = e;
    }
    RR_HIP(c, c->d_levels.ensure(order.size()));
    if (!order.empty()) RR_HIP(c, hipMemcpy(c->d_levels.p, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (!c->have_built) {
        RR_HIP(c, c->d_built.ensure(8 * nn));
        if (nn) RR_HIP(c, hipMemcpy(c->d_built.p, c->d_bvh.p, nn * sizeof(Node4), hipMemcpyDeviceToDevice));
        c->have_built = true; c->built_hit_pad = c->hit_pad;
    }
    if (!c->cost_known) {
        int rc = nn ? tree_cost(c, &c->cost_at_build) : 0; if (rc) return rc;
        c->cost_known = true;
    }
    c->dyn_ready = true;
    return 0;
}

// the extent reduction over the posed corners of (verts, poses), read back once: validates the call (every posed corner
// finite) and forms hit_pad with guard_pad's arithmetic and the box padding with the builders' rule
int refit_measure(rr_ctx* c, const float* d_verts, const float* d_poses, float* hit_pad, float* inflate, const char* who)
{
    *hit_pad = 0.f; *inflate = 1e-6f;
    if (c->n_tris == 0) return 0;
    const int G = refit_reduce_groups();
    RR_HIP(c, c->d_red.ensure((size_t)G * 8));
    launch_refit_extent(dev_tris(c), c->n_tris, d_verts, c->d_rest_f.p, d_poses, c->d_red.p, c->stream);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<float> part((size_t)G * 8);
    RR_HIP(c, hipMemcpy(part.data(), c->d_red.p, part.size() * sizeof(float), hipMemcpyDeviceToHost));
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    bool bad = false;
    for (int g = 0; g < G; g++) {
        const float* p = &part[(size_t)g * 8];
        for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[3 + k]); }
        bad |= p[6] != 0.0f;
    }
    if (bad) return fail(c, -3, std::string(who) + ": a posed vertex is not finite (nothing was changed)");
    float ext = 0.f, mag = 0.f;
    for (int k = 0; k < 3; k++) { ext = std::max(ext, hi[k] - lo[k]); mag = std::max(mag, std::max(std::fabs(lo[k]), std::fabs(hi[k]))); }
    *hit_pad = 1e-5f * std::max(ext, mag);                  // guard_pad
    *inflate = 2e-5f * std::max(ext, mag) + 1e-6f;          // build_bvh4 / build_bvh4_gpu
    return 0;
}

// the validated state -> the tree: triangle records, then the boxes level by level, deepest first
int refit_commit(rr_ctx* c, float hit_pad, float inflate)
{
    if (c->n_tris) {
        // which objects sit where the tree was built for them (same pose, same rest vertices)
        std::vector<uint8_t> moved(c->n_objects, 1);
        for (uint32_t o = 0; o < c->n_objects && !c->verts_dirty; o++)
            moved[o] = std::memcmp(&c->poses[7 * (size_t)o], &c->build_poses[7 * (size_t)o], 7 * sizeof(float)) != 0;
        RR_HIP(c, c->d_moved.ensure(moved.size()));
        RR_HIP(c, hipMemcpy(c->d_moved.p, moved.data(), moved.size(), hipMemcpyHostToDevice));
        // a grown extent grows the padding rule: the as-built boxes widen by the difference (2 x that of hit_pad, + 1 %)
        const float extra = hit_pad > c->built_hit_pad ? 2.0f * (hit_pad - c->built_hit_pad) * 1.01f : 0.0f;
        launch_refit_tris(dev_tris(c), c->n_tris, c->d_rest_v.p, c->d_rest_f.p, c->d_poses.p, c->stream);
        launch_refit_levels(c->d_bvh.p, c->d_levels.p, c->level_off.data(), (int)c->level_off.size() - 1, inflate,
                            c->d_built.p, c->d_moved.p, extra, c->stream);
        RR_HIP(c, hipGetLastError());
        RR_HIP(c, hipStreamSynchronize(c->stream));
    }
    // hit_pad travels by value in Params: captured launches bake it in.  Nothing else a launch holds changed (the tree
    // stays where it is, its depth and stack bound depend on its topology only), so a refit at the same extent keeps them
    if (hit_pad != c->hit_pad) c->graph_gen++;
    c->hit_pad = hit_pad;
    return 0;
}

// the finished host tree -> the ctx's one allocation (nodes, then triangles; references re-encoded as offsets)
int upload_tree(rr_ctx* c, const Bvh4& bvh)
{
    const size_t nn = bvh.nodes.size(), nt = bvh.tris.size();
    int rc = check_bvh_size(c, nn, nt); if (rc) return rc;
    // from here on the old tree is being overwritten: no mesh until the new one is complete (an error
    // return below leaves the context without a mesh, never with a half-written one)
    c->have_mesh = false;
    for (Lane& L : c->lanes) L.buf_seg = 0;
    c->tri_base4 = (uint32_t)(nn * 8);
    RR_HIP(c, c->d_bvh.ensure(nn * 8 + (nt + 4) * 3));   // +4 triangles: a quad may fetch past a short leaf
    RR_HIP(c, hipMemcpy(c->d_bvh.p, bvh.nodes.data(), nn * sizeof(Node4), hipMemcpyHostToDevice));
    if (nt) RR_HIP(c, hipMemcpy(c->d_bvh.p + c->tri_base4, bvh.tris.data(), nt * sizeof(TriRec), hipMemcpyHostToDevice));
    launch_encode_refs(reinterpret_cast<Node4*>(c->d_bvh.p), nn, c->tri_base4, nullptr, nt);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipDeviceSynchronize());
    c->n_nodes = nn; c->n_tris = nt;
    c->depth = bvh.depth; c->stack_need = bvh.stack_need;
    c->have_mesh = true; c->hist_gen++; c->graph_gen++;
    for (Lane& L : c->lanes) L.buf_seg = 0;   // stack geometry may have changed
    return 0;
}

// traversal steps (node + leaf) the uploaded tree costs a fixed sample of radar-like rays: origins in the middle of the
// map's footprint and the lower half of its height, directions within +-5 degrees of horizontal (a radar's beam; reflections
// off walls stay level) -- a deterministic sample, the same for every candidate tree of a mesh
int measure_tree_steps(rr_ctx* c, const float lo[3], const float hi[3], double* steps_per_ray)
{
    const int n = 16384;
    std::vector<float> o(3 * (size_t)n), d(3 * (size_t)n);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto u01 = [&]() { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((st >> 40) * (1.0 / 16777216.0)); };
    for (int i = 0; i < n; i++) {
        for (int k = 0; k < 2; k++) o[3 * i + k] = lo[k] + (0.25f + 0.5f * u01()) * (hi[k] - lo[k]);
        o[3 * i + 2] = lo[2] + (0.05f + 0.45f * u01()) * (hi[2] - lo[2]);
        const float yaw = 6.2831853f * u01(), el = (u01() - 0.5f) * 0.1745f;
        d[3 * i] = cosf(el) * cosf(yaw); d[3 * i + 1] = cosf(el) * sinf(yaw); d[3 * i + 2] = sinf(el);
    }
    const int stack_lds = (int)std::max<uint32_t>(1, std::min<uint32_t>(c->stack_need, (uint32_t)c->stack_lds_max));
    const int spill_depth = (int)c->stack_need - stack_lds;
    DevBuf<float> d_o, d_d; DevBuf<uint32_t> d_spill; DevBuf<unsigned long long> d_steps;
    RR_HIP(c, d_o.ensure(3 * (size_t)n));
    RR_HIP(c, d_d.ensure(3 * (size_t)n));
    RR_HIP(c, d_spill.ensure(spill_depth > 0 ? (size_t)spill_depth * n : 1));
    RR_HIP(c, d_steps.ensure(1));
    RR_HIP(c, hipMemcpy(d_o.p, o.data(), o.size() * sizeof(float), hipMemcpyHostToDevice));
    RR_HIP(c, hipMemcpy(d_d.p, d.data(), d.size() * sizeof(float), hipMemcpyHostToDevice));
    RR_HIP(c, hipMemset(d_steps.p, 0, sizeof(unsigned long long)));
    Params P; std::memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const Node4*>(c->d_bvh.p); P.tris = reinterpret_cast<const TriRec*>(c->d_bvh.p + c->tri_base4);
    P.tri_base4 = c->tri_base4; P.range_max = c->have_cfg ? c->cfg.range_max : 1000.0f; P.hit_pad = c->hit_pad;
    P.spill = d_spill.p; P.spill_stride = n; P.stack_lds = stack_lds; P.spill_depth = std::max(0, spill_depth);
    P.cull_pop = c->cull_pop;
    launch_debug_trace(P, d_o.p, d_d.p, n, nullptr, nullptr, c->stream, d_steps.p);
    RR_HIP(c, hipStreamSynchronize(c->stream));
    unsigned long long h = 0;
    RR_HIP(c, hipMemcpy(&h, d_steps.p, sizeof(h), hipMemcpyDeviceToHost));
    *steps_per_ray = (double)h / n;
    return 0;
}

}  // namespace

extern "C" {

int rr_set_mesh(rr_ctx* c, const float* verts, size_t nv, const uint32_t* faces, size_t nf,
                const uint32_t* face_object_id)
{
    if (!c) return -1;
    RR_HIP(c, hipSetDevice(c->device));
    Bvh4 bvh; std::string err;
    // Which tree?  The default -- SAH over references with spatial splits and the vertical weight (rr_bvh.h) -- halves the
    // traversal steps of maps that mix 0.2 m terrain with 10 m building faces, but on a small regular mesh its few
    // spatial splits disturb the packing (the 100k-triangle heightfield of config 2: 12.3 steps per ray against 10.9 for
    // the plain SAH).  Images do not depend on the tree, so for meshes that build in a fraction of a second the choice
    // is MEASURED: the candidates are uploaded one after the other, each traces the same sample of radar-like rays, the
    // one with the fewest traversal steps stays.  RR_BVH_CHOOSE=0 (or any RR_BVH_ALPHA / _WZ experiment): default only.
    const bool choose = nf > 0 && nf <= (size_t)2000000 && !(getenv("RR_BVH_CHOOSE") && atoi(getenv("RR_BVH_CHOOSE")) == 0) &&
                        !getenv("RR_BVH_ALPHA") && !getenv("RR_BVH_WZ");
    // the builder allocates hundreds of MB and starts threads: whatever it throws (bad_alloc, system_error) stops here
    try {
    if (!build_bvh4(verts, nv, faces, nf, face_object_id, bvh, err)) return fail(c, -4, err);
    if (bvh.spatial_splits > 0 && bvh.nodes.size() * 8 + (bvh.tris.size() + 4) * 3 >= (1ull << 28)) {
        // the parts spatial splits add pushed the tree over the 28-bit reference range: build without them
        BvhOptions plain; plain.sbvh_alpha = -1.0f;
        if (!build_bvh4(verts, nv, faces, nf, face_object_id, bvh, err, 0, &plain)) return fail(c, -4, err);
    }
    // frames in flight on the lane streams or a caller's stream (all non-blocking: a blocking hipMemcpy
    // does not order against them) still trace the old tree
    RR_HIP(c, hipDeviceSynchronize());
    c->hit_pad = guard_pad(verts, faces, nf);       // (build_bvh4 has checked the indices)
    int rc = upload_tree(c, bvh); if (rc) return rc;
    if (choose) {
        float lo[3] = { 3e38f, 3e38f, 3e38f }, hi[3] = { -3e38f, -3e38f, -3e38f };
        for (size_t i = 0; i < nv; i++) for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], verts[3 * i + k]); hi[k] = std::max(hi[k], verts[3 * i + k]); }
        double best = 0.0;
        rc = measure_tree_steps(c, lo, hi, &best); if (rc) return rc;
        const bool verbose = getenv("RR_BVH_VERBOSE") != nullptr;
        if (verbose) fprintf(stderr, "[rr bvh] tree choice: SAH + spatial splits, vertical weight 0.5: %.2f steps per sample ray\n", best);
        int kept = 0;
        for (int cand = 1; cand <= 2; cand++) {
            BvhOptions o; o.sbvh_alpha = -1.0f; o.vertical_weight = cand == 1 ? 0.5f : 1.0f;
            Bvh4 alt;
            if (!build_bvh4(verts, nv, faces, nf, face_object_id, alt, err, 0, &o)) continue;
            rc = upload_tree(c, alt); if (rc) return rc;
            double st = 0.0;
            rc = measure_tree_steps(c, lo, hi, &st); if (rc) return rc;
            if (verbose) fprintf(stderr, "[rr bvh] tree choice: plain SAH, vertical weight %.1f: %.2f steps per sample ray\n", o.vertical_weight, st);
            if (st < best * 0.98) { best = st; kept = cand; bvh = std::move(alt); }      // (2 %: do not trade trees over noise in the sample)
        }
        if (kept != 2) { rc = upload_tree(c, bvh); if (rc) return rc; }                  // the last candidate uploaded is not the winner
        if (verbose) fprintf(stderr, "[rr bvh] tree choice: kept candidate %d\n", kept);
    }
    } catch (const std::exception& ex) { c->have_mesh = false; return fail(c, -4, std::string("rr_set_mesh: host BVH build failed: ") + ex.what());
    } catch (...) { c->have_mesh = false; return fail(c, -4, "rr_set_mesh: host BVH build failed"); }
    return keep_rest(c, verts, nv, faces, nf, face_object_id);
}

int rr_set_mesh_gpu(rr_ctx* c, const float* verts, size_t nv, const uint32_t* faces, size_t nf,
                    const uint32_t* face_object_id)
{
    if (!c) return -1;
    if (nf == 0) return rr_set_mesh(c, verts, nv, faces, nf, face_object_id);
    if (!verts || !faces) return fail(c, -4, "rr_set_mesh_gpu: null vertex/face pointer");
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());
    Node4* dn = nullptr; TriRec* dt = nullptr; size_t nn = 0, nt = 0; uint32_t depth = 0, need = 0; float inflate = 0.f;
    std::string err;
    if (!build_bvh4_gpu(verts, nv, faces, nf, face_object_id, &dn, &nn, &dt, &nt, &depth, &need, &inflate, err, c->stream))
        return fail(c, -4, err);
    {
        // the builder hands over two arrays: move them into the one allocation the traversal addresses
        int rc = check_bvh_size(c, nn, nt);
        hipError_t e = hipSuccess;
        if (!rc) {
            c->have_mesh = false;           // see rr_set_mesh: no mesh while the tree is being replaced
            for (Lane& L : c->lanes) L.buf_seg = 0;
            c->tri_base4 = (uint32_t)(nn * 8);
            e = c->d_bvh.ensure(nn * 8 + (nt + 4) * 3);
            if (e == hipSuccess) e = hipMemcpy(c->d_bvh.p, dn, nn * sizeof(Node4), hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipMemcpy(c->d_bvh.p + c->tri_base4, dt, nt * sizeof(TriRec), hipMemcpyDeviceToDevice);
        }
        (void)hipFree(dn); (void)hipFree(dt);
        if (rc) return rc;
        RR_HIP(c, e);
        launch_encode_refs(reinterpret_cast<Node4*>(c->d_bvh.p), nn, c->tri_base4, nullptr, nt);
        RR_HIP(c, hipGetLastError());
        RR_HIP(c, hipDeviceSynchronize());
    }
    c->n_nodes = nn; c->n_tris = nt; c->depth = depth; c->stack_need = need;
    c->hit_pad = guard_pad(verts, faces, nf);
    c->have_mesh = true; c->hist_gen++; c->graph_gen++;
    for (Lane& L : c->lanes) L.buf_seg = 0;
    return keep_rest(c, verts, nv, faces, nf, face_object_id);
}

int rr_copy_mesh(rr_ctx* c, rr_ctx* src)
{
    if (!c) return -1;
    if (!src || src == c) return fail(c, -3, "rr_copy_mesh: need another context as the source");
    if (!src->have_mesh) return fail(c, -2, "rr_copy_mesh: the source context has no mesh");
    // nothing may still trace the old tree here, nothing may still write the source's
    RR_HIP(c, hipSetDevice(src->device));
    RR_HIP(c, hipDeviceSynchronize());
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());
    const size_t n4 = (size_t)src->n_nodes * 8 + ((size_t)src->n_tris + 4) * 3;     // float4 records, as rr_set_mesh sizes them
    c->have_mesh = false;
    for (Lane& L : c->lanes) L.buf_seg = 0;
    RR_HIP(c, c->d_bvh.ensure(n4));
    // child references are offsets from the base of the allocation: the tree is position independent
    if (src->device == c->device) RR_HIP(c, hipMemcpy(c->d_bvh.p, src->d_bvh.p, n4 * sizeof(float4), hipMemcpyDeviceToDevice));
    else RR_HIP(c, hipMemcpyPeer(c->d_bvh.p, c->device, src->d_bvh.p, src->device, n4 * sizeof(float4)));
    RR_HIP(c, hipDeviceSynchronize());
    c->tri_base4 = src->tri_base4; c->n_nodes = src->n_nodes; c->n_tris = src->n_tris;
    c->depth = src->depth; c->stack_need = src->stack_need; c->hit_pad = src->hit_pad;
    // the rest geometry and the poses too: the copy can be posed on its own
    RR_HIP(c, c->d_rest_v.ensure(3 * src->rest_nv));
    RR_HIP(c, c->d_rest_f.ensure(3 * src->rest_nf));
    RR_HIP(c, c->d_poses.ensure(src->poses.size()));
    if (src->device == c->device) {
        RR_HIP(c, hipMemcpy(c->d_rest_v.p, src->d_rest_v.p, 3 * src->rest_nv * sizeof(float), hipMemcpyDeviceToDevice));
        RR_HIP(c, hipMemcpy(c->d_rest_f.p, src->d_rest_f.p, 3 * src->rest_nf * sizeof(uint32_t), hipMemcpyDeviceToDevice));
    } else {
        RR_HIP(c, hipMemcpyPeer(c->d_rest_v.p, c->device, src->d_rest_v.p, src->device, 3 * src->rest_nv * sizeof(float)));
        RR_HIP(c, hipMemcpyPeer(c->d_rest_f.p, c->device, src->d_rest_f.p, src->device, 3 * src->rest_nf * sizeof(uint32_t)));
    }
    RR_HIP(c, hipMemcpy(c->d_poses.p, src->poses.data(), src->poses.size() * sizeof(float), hipMemcpyHostToDevice));
    c->rest_nv = src->rest_nv; c->rest_nf = src->rest_nf; c->n_objects = src->n_objects; c->poses = src->poses;
    c->twists.assign(6 * (size_t)src->n_objects, 0.0f);
    c->d_stage_v.release(); c->d_stage_poses.release();
    c->dyn_ready = false; c->cost_known = src->cost_known; c->cost_at_build = src->cost_at_build;
    c->build_poses = src->build_poses; c->verts_dirty = src->verts_dirty; c->have_built = false;
    if (src->have_built) {          // the source has refit its tree already: its snapshot is what the builder made
        RR_HIP(c, c->d_built.ensure(8 * (size_t)src->n_nodes));
        if (src->device == c->device) RR_HIP(c, hipMemcpy(c->d_built.p, src->d_built.p, src->n_nodes * sizeof(Node4), hipMemcpyDeviceToDevice));
        else RR_HIP(c, hipMemcpyPeer(c->d_built.p, c->device, src->d_built.p, src->device, src->n_nodes * sizeof(Node4)));
        c->have_built = true; c->built_hit_pad = src->built_hit_pad;
    }
    c->have_mesh = true; c->hist_gen++; c->graph_gen++;
    return 0;
}

// ---- dynamic scenes (rr_refit.hip) ----------------------------------------------------------------------------------
int rr_set_object_poses(rr_ctx* c, const float* poses, size_t n)
{
    if (!c) return -1;
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    if (!poses) return fail(c, -3, "rr_set_object_poses: null poses");
    if (n != c->n_objects)
        return fail(c, -3, "rr_set_object_poses: expected " + std::to_string(c->n_objects) + " poses (one per object), got " + std::to_string(n));
    for (size_t i = 0; i < 7 * n; i++) if (!std::isfinite(poses[i])) return fail(c, -3, "rr_set_object_poses: non-finite pose value");
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());       // work in flight renders the old scene
    int rc = refit_prepare(c); if (rc) return rc;
    RR_HIP(c, c->d_stage_poses.ensure(7 * n));
    RR_HIP(c, hipMemcpy(c->d_stage_poses.p, poses, 7 * n * sizeof(float), hipMemcpyHostToDevice));
    float hp = 0.f, inflate = 0.f;
    rc = refit_measure(c, c->d_rest_v.p, c->d_stage_poses.p, &hp, &inflate, "rr_set_object_poses"); if (rc) return rc;
    std::swap(c->d_poses, c->d_stage_poses);
    c->poses.assign(poses, poses + 7 * n);
    return refit_commit(c, hp, inflate);
}

int rr_set_object_twists(rr_ctx* c, const float* twists, size_t n)
{
    if (!c) return -1;
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    if (n != 0 && n != c->n_objects)
        return fail(c, -3, "rr_set_object_twists: expected " + std::to_string(c->n_objects) + " twists (one per object) or 0, got " + std::to_string(n));
    if (n != 0 && !twists) return fail(c, -3, "rr_set_object_twists: null twists");
    for (size_t i = 0; i < 6 * n; i++) if (!std::isfinite(twists[i])) return fail(c, -3, "rr_set_object_twists: non-finite twist value");
    // by value: the next Doppler call carries them down with its own arguments -- nothing is drained, no tree or launch graph is touched
    if (n == 0) c->twists.assign(6 * (size_t)c->n_objects, 0.0f);
    else c->twists.assign(twists, twists + 6 * n);
    return 0;
}

int rr_update_vertices(rr_ctx* c, const float* verts, size_t nv)
{
    if (!c) return -1;
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    if (!verts) return fail(c, -3, "rr_update_vertices: null vertices");
    if (nv != c->rest_nv)
        return fail(c, -3, "rr_update_vertices: expected " + std::to_string(c->rest_nv) + " vertices (the mesh's), got " + std::to_string(nv));
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());
    int rc = refit_prepare(c); if (rc) return rc;
    RR_HIP(c, c->d_stage_v.ensure(3 * nv));
    if (nv) RR_HIP(c, hipMemcpy(c->d_stage_v.p, verts, 3 * nv * sizeof(float), hipMemcpyHostToDevice));
    float hp = 0.f, inflate = 0.f;
    rc = refit_measure(c, c->d_stage_v.p, c->d_poses.p, &hp, &inflate, "rr_update_vertices"); if (rc) return rc;
    std::swap(c->d_rest_v, c->d_stage_v);
    c->verts_dirty = true;          // (the same values count as new: the builder's clipped boxes are not checked against them)
    return refit_commit(c, hp, inflate);
}

int rr_get_tree_cost(rr_ctx* c, double* cost_now, double* cost_at_build)
{
    if (!c) return -1;
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    RR_HIP(c, hipSetDevice(c->device));
    int rc = refit_prepare(c); if (rc) return rc;
    double now = 0.0;
    if (c->n_nodes) { rc = tree_cost(c, &now); if (rc) return rc; }
    if (cost_now) *cost_now = now;
    if (cost_at_build) *cost_at_build = c->cost_at_build;
    return 0;
}

int rr_rebuild_tree(rr_ctx* c, int builder)
{
    if (!c) return -1;
    if (builder != 0 && builder != 1) return fail(c, -3, "rr_rebuild_tree: builder must be 0 (host SAH) or 1 (GPU LBVH)");
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());
    const size_t nf = c->rest_nf;
    if (nf == 0 || c->n_tris == 0) return 0;
    // the posed soup (face order, corners 3f .. 3f + 2) and its object ids, to the host: both builders take host arrays
    std::vector<float> soup(9 * nf);
    std::vector<uint32_t> obj(nf), faces(3 * nf);
    {
        DevBuf<float> d_soup; DevBuf<uint32_t> d_obj;
        RR_HIP(c, d_soup.ensure(9 * nf));
        RR_HIP(c, d_obj.ensure(nf));
        launch_pose_soup(dev_tris(c), c->n_tris, c->d_rest_v.p, c->d_rest_f.p, c->d_poses.p, d_soup.p, d_obj.p, c->stream);
        RR_HIP(c, hipGetLastError());
        RR_HIP(c, hipStreamSynchronize(c->stream));
        RR_HIP(c, hipMemcpy(soup.data(), d_soup.p, soup.size() * sizeof(float), hipMemcpyDeviceToHost));
        RR_HIP(c, hipMemcpy(obj.data(), d_obj.p, obj.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    for (size_t i = 0; i < 3 * nf; i++) faces[i] = (uint32_t)i;
    // the build replaces the tree (and bumps graph_gen: the tree moves); the rest data, the poses and the trace-grid
    // history stay -- wave counts do not depend on the tree
    const int hist = c->hist_gen;
    c->rebuilding = true;
    const int rc = builder == 0 ? rr_set_mesh(c, soup.data(), 3 * nf, faces.data(), nf, obj.data())
                                : rr_set_mesh_gpu(c, soup.data(), 3 * nf, faces.data(), nf, obj.data());
    c->rebuilding = false;
    c->hist_gen = hist;
    return rc;
}

int rr_get_bvh_info(rr_ctx* c, uint64_t* n_nodes, uint64_t* n_tris, uint32_t* depth, uint32_t* stack_need)
{
    if (!c) return -1;
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    if (n_nodes) *n_nodes = c->n_nodes;
    if (n_tris) *n_tris = c->n_tris;
    if (depth) *depth = c->depth;
    if (stack_need) *stack_need = c->stack_need;
    return 0;
}

}  // extern "C"
