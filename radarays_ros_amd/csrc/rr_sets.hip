// rr_sets.hip -- parameter batches: ONE pose under several parameter sets (material tables, beam samples, passes) in one launch chain, with optional scores
#include "rr_stage.h"
#include <algorithm>
#include <cmath>
#include <cstring>

extern "C" {

int rr_simulate_param_sets_device(rr_ctx* c, const float pose[7], const rr_param_set* sets, int n_sets, size_t n_materials,
                                  uint8_t* d_imgs_u8, void* stream)
{
    int rc = check_ready(c); if (rc) return rc;
    if (!pose || !sets || !d_imgs_u8) return fail(c, -3, "rr_simulate_param_sets_device: null pose/sets/output");
    if (n_sets < 1 || n_sets > RR_MAX_BATCH) return fail(c, -3, "rr_simulate_param_sets_device: n_sets must be 1..64");
    const size_t n_mat = c->materials.size();
    if (n_materials != n_mat)
        return fail(c, -3, "rr_simulate_param_sets_device: every set must hold as many materials as the table given to rr_set_materials");
    const size_t nb = c->beams.size() / 3;
    if (nb == 0) return fail(c, -2, "rr_set_beam_samples has not been called");
    int p_max = 0;
    SetPlan plan; plan.n_groups = 0;
    std::vector<const float*> group_dirs;         // beam table of each group (null: the ctx's own samples)
    for (int k = 0; k < n_sets; k++) {
        const rr_param_set& S = sets[k];
        const int np = S.n_reflections < 0 ? c->cfg.n_reflections : S.n_reflections;
        if (np > 16) return fail(c, -3, "rr_simulate_param_sets_device: n_reflections must be <= 16 (negative: the config's)");
        p_max = std::max(p_max, np);
        plan.frame_passes[k] = (unsigned char)np;
        if (S.materials)
            for (size_t i = 0; i < n_mat; i++)
                if (!std::isfinite(S.materials[i].velocity) || !std::isfinite(S.materials[i].ambient) || !std::isfinite(S.materials[i].diffuse) ||
                    !std::isfinite(S.materials[i].specular))
                    return fail(c, -3, "rr_simulate_param_sets_device: non-finite material parameter");
        if (S.beam_dirs) for (size_t i = 0; i < 3 * nb; i++) if (!std::isfinite(S.beam_dirs[i])) return fail(c, -3, "rr_simulate_param_sets_device: non-finite beam direction");
        // sets with the same directions (the same pointer, or the same bytes) form a group and share pass 0
        const float* dirs = S.beam_dirs;
        if (dirs && std::memcmp(dirs, c->beams.data(), 3 * nb * sizeof(float)) == 0) dirs = nullptr;
        int g = -1;
        for (int j = 0; j < plan.n_groups && g < 0; j++) {
            const float* o = group_dirs[(size_t)j];
            if (o == dirs || (o && dirs && std::memcmp(o, dirs, 3 * nb * sizeof(float)) == 0)) g = j;
        }
        if (g < 0) { g = plan.n_groups++; group_dirs.push_back(dirs); plan.group_frame[g] = (unsigned char)k; }
        plan.frame_beam[k] = (unsigned char)g;
    }
    RR_HIP(c, hipSetDevice(c->device));
    const rr_config& g0 = c->cfg;
    hipStream_t s = stream_of(c, stream);
    rc = upload_tables(c); if (rc) return rc;
    const size_t li = c->next_lane++ % c->lanes.size();
    Lane& L = c->lanes[li];
    rc = take_lane(c, li, s); if (rc) return rc;
    static_assert(sizeof(rr_material) == sizeof(float4), "rr_material is {velocity, ambient, diffuse, specular}");
    const size_t G = (size_t)plan.n_groups;
    const bool own_beams = !(G == 1 && group_dirs[0] == nullptr);
    if (L.d_matsets.n < (size_t)n_sets * n_mat || (own_beams && L.d_set_beams.n < G * nb)) {
        RR_HIP(c, hipDeviceSynchronize());      // the tables of this lane may still be read by an earlier step
        RR_HIP(c, L.d_matsets.ensure((size_t)n_sets * n_mat));
        RR_HIP(c, L.d_matset_limits.ensure((size_t)n_sets * n_mat));
        if (own_beams) { RR_HIP(c, L.d_set_beams.ensure(G * nb)); RR_HIP(c, L.d_set_order.ensure(G * nb)); RR_HIP(c, L.d_set_order2.ensure(G * nb)); }
    }
    // the lane's previous use of these host arrays: its copies were enqueued on a stream this stream now waits for
    // (ev_consumed), but a staged copy reads the host side at an unknown time: wait for the lane's last batch before reuse
    if (L.pending_consume) RR_HIP(c, hipEventSynchronize(L.ev_consumed));
    L.h_matsets.resize((size_t)n_sets * n_mat);
    for (int k = 0; k < n_sets; k++) {
        const rr_material* m = sets[k].materials ? sets[k].materials : c->materials.data();
        for (size_t i = 0; i < n_mat; i++) L.h_matsets[(size_t)k * n_mat + i] = make_float4(m[i].velocity, m[i].ambient, m[i].diffuse, m[i].specular);
    }
    if (own_beams) {
        L.h_set_beams.resize(G * nb); L.h_set_order.resize(G * nb); L.h_set_order2.resize(G * nb);
        std::vector<uint32_t> o1, o2;
        for (size_t gi = 0; gi < G; gi++) {
            const float* d = group_dirs[gi] ? group_dirs[gi] : c->beams.data();
            for (size_t i = 0; i < nb; i++) L.h_set_beams[gi * nb + i] = make_float4(d[3 * i], d[3 * i + 1], d[3 * i + 2], 0.0f);
            beam_trace_orders(d, nb, o1, o2);
            std::copy(o1.begin(), o1.end(), L.h_set_order.begin() + (std::ptrdiff_t)(gi * nb));
            std::copy(o2.begin(), o2.end(), L.h_set_order2.begin() + (std::ptrdiff_t)(gi * nb));
        }
        plan.d_beams = L.d_set_beams.p; plan.d_order = L.d_set_order.p; plan.d_order2 = L.d_set_order2.p;
    }
    // sizes follow the largest number of passes of the batch
    c->passes_override = p_max;
    rc = prepare_lane(c, L, n_sets * g0.n_angles);
    if (!rc) {
        hipError_t e = hipMemcpyAsync(L.d_matsets.p, L.h_matsets.data(), L.h_matsets.size() * sizeof(float4), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && own_beams) e = hipMemcpyAsync(L.d_set_beams.p, L.h_set_beams.data(), G * nb * sizeof(float4), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && own_beams) e = hipMemcpyAsync(L.d_set_order.p, L.h_set_order.data(), G * nb * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && own_beams) e = hipMemcpyAsync(L.d_set_order2.p, L.h_set_order2.data(), G * nb * sizeof(uint32_t), hipMemcpyHostToDevice, s);
        if (e != hipSuccess) rc = fail(c, -100, std::string("rr_simulate_param_sets_device: ") + hipGetErrorString(e));
    }
    if (!rc) {
        launch_mat_limits(L.d_matsets.p, (size_t)n_sets * n_mat, L.d_matset_limits.p, s);
        FrameJob job; job.n_frames = n_sets; job.d_matsets = L.d_matsets.p; job.mat_stride = (int)n_mat; job.plan = &plan;
        rc = run_frame(c, L, pose, 0, g0.n_angles, s, job);
    }
    c->passes_override = -1;
    if (rc) {
        // staged copies from the lane's host vectors may already be enqueued (advisor, round 4): the next call on this lane
        // must not rewrite them underneath -- it waits for ev_consumed like after a complete batch
        (void)give_lane(L, s);
        return rc;
    }
    rc = assemble_frames(c, L, d_imgs_u8, n_sets, s); if (rc) return rc;
    RR_HIP(c, give_lane(L, s));
    return 0;
}

int rr_simulate_material_sets_device(rr_ctx* c, const float pose[7], const rr_material* sets, int n_sets,
                                     size_t n_materials, uint8_t* d_imgs_u8, void* stream)
{
    if (!c) return -1;
    if (!pose || !sets || !d_imgs_u8) return fail(c, -3, "rr_simulate_material_sets_device: null pose/sets/output");
    if (n_sets < 1 || n_sets > RR_MAX_BATCH) return fail(c, -3, "rr_simulate_material_sets_device: n_sets must be 1..64");
    if (n_materials != c->materials.size())
        return fail(c, -3, "rr_simulate_material_sets_device: every set must hold as many materials as the table given to rr_set_materials");
    // the parameter batch with only the material tables varying: one beam group, the config's passes
    rr_param_set ps[RR_MAX_BATCH];
    for (int k = 0; k < n_sets; k++) { ps[k].materials = sets + (size_t)k * n_materials; ps[k].beam_dirs = nullptr; ps[k].n_reflections = -1; ps[k].reserved_ = 0; }
    return rr_simulate_param_sets_device(c, pose, ps, n_sets, n_materials, d_imgs_u8, stream);
}

}  // extern "C"

namespace {
// The round trip the host forms share (rr_stage.h): `simulate(d_imgs)` runs a parameter batch into the stage's room; its images are scored
// and / or copied out, the latter once the frame's error bits have come home clean
template <class Simulate>
int param_batch_to_host(rr_ctx* c, int n_sets, Simulate simulate, uint8_t* out_imgs_u8, const uint8_t* ref_img_u8, double* out_psnr,
                        uint32_t which = 0, int win_size = 0, rr_image_metrics* out_metrics = nullptr)
{
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n = (size_t)n_sets;
    RR_STAGE(c, st);
    uint8_t *d_imgs, *d_ref;
    RR_HIP(c, st.room(n * npx, d_imgs));
    RR_HIP(c, st.up(out_psnr || out_metrics ? ref_img_u8 : nullptr, npx, d_ref));
    int rc = simulate(d_imgs); if (rc) return rc;
    // (both synchronise the stream)
    if (d_ref && out_psnr) rc = rr_score_images_device(c, d_imgs, n_sets, d_ref, out_psnr, nullptr, c->stream);
    if (d_ref && out_metrics && !rc) rc = rr_compare_images_device(c, d_imgs, n_sets, d_ref, which, win_size, out_metrics, nullptr, c->stream);
    if (rc) return rc;
    st.out(out_imgs_u8, d_imgs, n * npx, false);
    return st.commit([c] { return report_frame_errors(c); });
}
}  // namespace

extern "C" {

int rr_simulate_material_sets(rr_ctx* c, const float pose[7], const rr_material* sets, int n_sets, size_t n_materials,
                              uint8_t* out_imgs_u8)
{
    if (!c) return -1;
    if (!out_imgs_u8) return fail(c, -3, "rr_simulate_material_sets: null output");
    if (n_sets < 1 || n_sets > RR_MAX_BATCH) return fail(c, -3, "rr_simulate_material_sets: n_sets must be 1..64");
    return param_batch_to_host(c, n_sets, [&](uint8_t* d_imgs) {
        return rr_simulate_material_sets_device(c, pose, sets, n_sets, n_materials, d_imgs, c->stream); }, out_imgs_u8, nullptr, nullptr);
}

int rr_simulate_param_sets(rr_ctx* c, const float pose[7], const rr_param_set* sets, int n_sets, size_t n_materials,
                           uint8_t* out_imgs_u8, const uint8_t* ref_img_u8, double* out_psnr)
{
    if (!c) return -1;
    if (!out_imgs_u8 && !(ref_img_u8 && out_psnr)) return fail(c, -3, "rr_simulate_param_sets: neither an image buffer nor a reference image + score buffer");
    if ((ref_img_u8 == nullptr) != (out_psnr == nullptr)) return fail(c, -3, "rr_simulate_param_sets: ref_img_u8 and out_psnr go together");
    if (n_sets < 1 || n_sets > RR_MAX_BATCH) return fail(c, -3, "rr_simulate_param_sets: n_sets must be 1..64");
    return param_batch_to_host(c, n_sets, [&](uint8_t* d_imgs) {
        return rr_simulate_param_sets_device(c, pose, sets, n_sets, n_materials, d_imgs, c->stream); }, out_imgs_u8, ref_img_u8, out_psnr);
}

int rr_simulate_param_sets_metrics(rr_ctx* c, const float pose[7], const rr_param_set* sets, int n_sets, size_t n_materials,
                                   uint8_t* out_imgs_u8, const uint8_t* ref_img_u8, uint32_t which, int win_size, rr_image_metrics* out)
{
    // refused before anything is simulated (the context stands in for the images: they are its own)
    int rc = check_compare(c, "rr_simulate_param_sets_metrics", c, 1, ref_img_u8, which, win_size, out, nullptr); if (rc) return rc;
    if (n_sets < 1 || n_sets > RR_MAX_BATCH) return fail(c, -3, "rr_simulate_param_sets_metrics: n_sets must be 1..64");
    return param_batch_to_host(c, n_sets, [&](uint8_t* d_imgs) {
        return rr_simulate_param_sets_device(c, pose, sets, n_sets, n_materials, d_imgs, c->stream); }, out_imgs_u8, ref_img_u8, nullptr, which, win_size, out);
}

}  // extern "C"
