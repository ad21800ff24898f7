// marshal.hpp -- the marshalling between the state of a `Radar` object and the C ABI, stated once.
//
// Both C++ classes named RadarHIP use it: the ROS-free one (RadarHIP.hpp next to this file) and the ROS-typed adapter
// (integration/src/radarays_ros/RadarHIP.cpp).  The adapter cannot be built or run without ROS, so what runs on the GPU
// under tests/cpp/radar_hip_demo.cpp is this header, instantiated with the plain structs of the ROS-free class; the adapter
// instantiates the same templates with catkin's generated types.  No ROS / OpenCV / rmagine types, nothing is printed:
// a failure comes back as `false` (and a reason where there is a choice), each class reports it its own way.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../radarays_mi355.h"

namespace radarays_ros_amd::marshal {

// cfg/RadarModel.cfg fields + the constants of Radar::Radar (Radar.cpp:22-32) -> rr_config.  Cfg: the dynamic-reconfigure
// struct (generated or plain).  n_angles / theta_min / theta_inc keep rr_default_config's values: the caller's to set.
template <typename Cfg>
void fill_config(rr_config& c, const Cfg& cfg, int n_reflections, float wave_energy_threshold)
{
    rr_default_config(&c);
    c.n_cells = cfg.n_cells;
    c.n_reflections = n_reflections;
    c.signal_denoising = cfg.signal_denoising;
    c.signal_denoising_triangular_width = cfg.signal_denoising_triangular_width;
    c.signal_denoising_triangular_mode = cfg.signal_denoising_triangular_mode;
    c.signal_denoising_gaussian_width = cfg.signal_denoising_gaussian_width;
    c.signal_denoising_gaussian_mode = cfg.signal_denoising_gaussian_mode;
    c.signal_denoising_mb_width = cfg.signal_denoising_mb_width;
    c.signal_denoising_mb_mode = cfg.signal_denoising_mb_mode;
    c.ambient_noise = cfg.ambient_noise;
    c.scroll_image = cfg.scroll_image;
    c.record_multi_reflection = cfg.record_multi_reflection;
    c.record_multi_path = cfg.record_multi_path;
    c.multipath_threshold = cfg.multipath_threshold;
    c.resolution = cfg.resolution;
    c.energy_max = cfg.energy_max;
    c.signal_max = cfg.signal_max;
    c.ambient_noise_at_signal_0 = cfg.ambient_noise_at_signal_0;
    c.ambient_noise_at_signal_1 = cfg.ambient_noise_at_signal_1;
    c.ambient_noise_energy_max = cfg.ambient_noise_energy_max;
    c.ambient_noise_energy_min = cfg.ambient_noise_energy_min;
    c.ambient_noise_energy_loss = cfg.ambient_noise_energy_loss;
    c.wave_energy_threshold = wave_energy_threshold;
    c.range_max = 1000.0f;     // make_model gives every pass's OnDn model range [0, 1000] (radar_algorithms.cpp:157-158)
}

// RadarMaterial (msg/RadarMaterial.msg, or the plain struct) -> rr_material, appended
template <typename It>
void append_materials(std::vector<rr_material>& out, It first, It last)
{
    for (; first != last; ++first) {
        const auto& m = *first;
        out.push_back({ m.velocity, m.ambient, m.diffuse, m.specular });
    }
}
// m_object_materials (Radar.hpp:97) as the ABI takes it
inline std::vector<int32_t> object_material_ids(const std::vector<int>& ids) { return { ids.begin(), ids.end() }; }

// sample_cone_local (RadarCPU.cpp:136-145) on a given seed: dirs = [n_samples][3].  Where the seed comes from is the
// caller's policy; false: beam_sample_dist is not one of 0..3
inline bool draw_beam(uint32_t seed, float beam_width, size_t n_samples, int dist, float p_in_cone, std::vector<float>& dirs)
{
    dirs.assign(3 * n_samples, 0.0f);
    return rr_sample_cone_local(seed, beam_width, n_samples, dist, p_in_cone, dirs.data()) == 0;
}

// Offline generation: n_frames frames in chunks of RR_MAX_BATCH, one set of launches per chunk.  poses = [n_frames][7], or
// with `sweeps` [n_frames][n_angles][7] (include_motion, RadarCPU.cpp:190-196): row k of a chunk's table = the per-azimuth
// poses of its frame k.  emit(pixels, frame) is called once per finished frame, pixels = npx bytes valid during the call.
// Returns whether it ran to the end; if not, rr_multi_last_error(m) says why.  A sweep table stays installed afterwards.
template <typename Emit>
bool render_chunks(rr_multi* m, const float* poses, size_t n_frames, bool sweeps, int n_angles, size_t npx, Emit emit)
{
    const size_t per = sweeps ? 7 * (size_t)n_angles : 7;
    std::vector<uint8_t> px((size_t)RR_MAX_BATCH * npx);
    std::vector<float> first;
    for (size_t at = 0; at < n_frames; at += RR_MAX_BATCH) {
        const size_t n = std::min(n_frames - at, (size_t)RR_MAX_BATCH);
        const float* p = poses + at * per;
        if (sweeps) {      // the pose arguments are ignored while a table is set, but must be valid: each frame's first pose
            first.clear();
            for (size_t k = 0; k < n; k++) first.insert(first.end(), p + k * per, p + k * per + 7);
            if (rr_multi_set_motion_poses(m, p, n * (size_t)n_angles)) return false;
        } else if (rr_multi_set_motion_poses(m, nullptr, 0)) return false;
        if (rr_multi_simulate_batch(m, sweeps ? first.data() : p, (int)n, px.data())) return false;
        for (size_t k = 0; k < n; k++) emit(px.data() + k * npx, at + k);
    }
    return true;
}

// The optimiser's parameter vectors (scripts/radaray_opti.py:36-113) as rr_simulate_param_sets takes them; owns what the
// rr_param_set array points into
struct ParamSetBatch {
    std::vector<rr_material> mats;            // [n_sets][n_mat]
    std::vector<std::vector<float>> dirs;     // per set: empty = the current beam, else its own draw
    std::vector<rr_param_set> ps;

    // sets: RadarParams-like (.model.beam_width / .n_samples / .n_reflections); materials_of(set) gives its material list.
    // Every set needs n_mat materials and n_beam samples.  A set whose beam_width differs from the current one gets its
    // own draw on `seed` -- the seed of the current beam, so that sets which differ only in beam_width share their variates
    template <typename Sets, typename MaterialsOf>
    bool build(const Sets& sets, MaterialsOf materials_of, size_t n_mat, size_t n_beam, float current_beam_width,
               uint32_t seed, int dist, float p_in_cone, std::string& why)
    {
        mats.clear(); dirs.clear(); ps.clear();
        dirs.resize(sets.size()); ps.resize(sets.size());
        for (size_t k = 0; k < sets.size(); k++) {
            const auto& p = sets[k];
            const auto& list = materials_of(p);
            if (list.size() != n_mat || p.model.n_samples != n_beam) { why = "every parameter set needs the loaded number of materials and the current n_samples"; return false; }
            append_materials(mats, list.begin(), list.end());
            if (std::abs(p.model.beam_width - current_beam_width) > 1e-7f &&
                !draw_beam(seed, p.model.beam_width, n_beam, dist, p_in_cone, dirs[k])) { why = "sample_cone_local failed"; return false; }
            ps[k].n_reflections = (int32_t)p.model.n_reflections; ps[k].reserved_ = 0;
        }
        for (size_t k = 0; k < sets.size(); k++) {      // only now: mats no longer moves
            ps[k].materials = mats.data() + k * n_mat;
            ps[k].beam_dirs = dirs[k].empty() ? nullptr : dirs[k].data();
        }
        return true;
    }
    // one pose -> ps.size() images [n_sets][npx] and / or their PSNR against `real` (each may be null); false: rr_last_error(ctx)
    bool run(rr_ctx* ctx, const float pose[7], size_t n_mat, uint8_t* pixels, const uint8_t* real, double* psnr) const
    {
        return rr_simulate_param_sets(ctx, pose, ps.data(), (int)ps.size(), n_mat, pixels, real, psnr) == 0;
    }
    // the same with any of the image metrics as the objective: one record per set against `real` (pixels may be null)
    bool run_metrics(rr_ctx* ctx, const float pose[7], size_t n_mat, uint8_t* pixels, const uint8_t* real, uint32_t which, int win_size,
                     rr_image_metrics* out) const
    {
        return rr_simulate_param_sets_metrics(ctx, pose, ps.data(), (int)ps.size(), n_mat, pixels, real, which, win_size, out) == 0;
    }
};

// n mono8 images (each npx bytes, wherever they lie) against one real image: one record per image.  image_pixels(k) gives
// image k's bytes.  false: rr_last_error(ctx)
template <typename PixelsOf>
bool compare_images(rr_ctx* ctx, size_t n, size_t npx, PixelsOf image_pixels, const uint8_t* real, uint32_t which, int win_size,
                    std::vector<rr_image_metrics>& out)
{
    std::vector<uint8_t> flat(n * npx);
    for (size_t k = 0; k < n; k++) std::copy(image_pixels(k), image_pixels(k) + npx, flat.begin() + (std::ptrdiff_t)(k * npx));
    out.assign(n, rr_image_metrics{});
    return rr_compare_images(ctx, flat.data(), (int)n, real, which, win_size, out.data(), nullptr) == 0;
}

// the same images registered against the real one along the azimuth axis (rr_align_images): one record per image over the cell
// window [cell_begin, cell_end), and with `curve` xcorr at every shift, [n][n_angles].  false: rr_last_error(ctx)
template <typename PixelsOf>
bool align_images(rr_ctx* ctx, size_t n, size_t npx, size_t n_angles, PixelsOf image_pixels, const uint8_t* real, int cell_begin, int cell_end,
                  std::vector<rr_align_record>& out, std::vector<int64_t>* curve)
{
    std::vector<uint8_t> flat(n * npx);
    for (size_t k = 0; k < n; k++) std::copy(image_pixels(k), image_pixels(k) + npx, flat.begin() + (std::ptrdiff_t)(k * npx));
    out.assign(n, rr_align_record{});
    if (curve) curve->assign(n * n_angles, 0);
    return rr_align_images(ctx, flat.data(), (int)n, real, cell_begin, cell_end, out.data(), curve ? curve->data() : nullptr) == 0;
}

// the same images and the real one made Cartesian (rr_polar_to_cartesian: width x width, pixel_size m/pixel) and registered over
// -max_shift..max_shift pixels (rr_shift_images): one record per image, and with `correction` the amount to add to each image's
// pose in the sensor's own axes, metres [n][2] = (forward, left) = ((dy + sub_dy), (dx + sub_dx)) * pixel_size.  false: rr_last_error(ctx)
template <typename PixelsOf>
bool register_translation(rr_ctx* ctx, size_t n, size_t npx, PixelsOf image_pixels, const uint8_t* real, int width, float pixel_size, int max_shift,
                          bool bilinear, std::vector<rr_shift_record>& out, std::vector<double>* correction)
{
    std::vector<uint8_t> flat((n + 1) * npx);           // the real image rides behind the others: one conversion
    for (size_t k = 0; k < n; k++) std::copy(image_pixels(k), image_pixels(k) + npx, flat.begin() + (std::ptrdiff_t)(k * npx));
    std::copy(real, real + npx, flat.begin() + (std::ptrdiff_t)(n * npx));
    rr_cartesian_config cc{};
    cc.width = width; cc.interpolation = bilinear ? 1 : 0; cc.pixel_size = pixel_size;
    const size_t ncart = width > 0 ? (size_t)width * (size_t)width : 0;
    std::vector<uint8_t> cart((n + 1) * ncart);
    out.assign(n, rr_shift_record{});
    if (rr_polar_to_cartesian(ctx, flat.data(), (int)(n + 1), &cc, cart.data()) != 0) return false;
    if (rr_shift_images(ctx, cart.data(), (int)n, cart.data() + n * ncart, width, width, max_shift, out.data(), nullptr, nullptr) != 0) return false;
    if (correction) {
        correction->assign(2 * n, 0.0);
        for (size_t k = 0; k < n; k++) {
            (*correction)[2 * k] = ((double)out[k].dy + out[k].sub_dy) * (double)pixel_size;
            (*correction)[2 * k + 1] = ((double)out[k].dx + out[k].sub_dx) * (double)pixel_size;
        }
    }
    return true;
}

// place recognition (rr_place_config, rr_place_match): the same images as ring/sector descriptors, [n][n_rings][n_sectors] bytes
// (rr_describe_images).  false: rr_last_error(ctx)
template <typename PixelsOf>
bool describe(rr_ctx* ctx, size_t n, size_t npx, PixelsOf image_pixels, const rr_place_config& cfg, std::vector<uint8_t>& desc)
{
    std::vector<uint8_t> flat(n * npx);
    for (size_t k = 0; k < n; k++) std::copy(image_pixels(k), image_pixels(k) + npx, flat.begin() + (std::ptrdiff_t)(k * npx));
    const size_t K = cfg.n_rings > 0 && cfg.n_sectors > 0 ? (size_t)cfg.n_rings * (size_t)cfg.n_sectors : 0;
    desc.assign(n * K, 0);
    return rr_describe_images(ctx, flat.data(), (int)n, &cfg, desc.data()) == 0;
}

// n_query descriptors against a database of n_db, all [n_rings][n_sectors] (rr_match_descriptors): the top_k candidates per query by
// (sse, index), [n_query][top_k].  false: rr_last_error(ctx)
inline bool match_places(rr_ctx* ctx, const uint8_t* query, size_t n_query, const uint8_t* db, size_t n_db, int n_rings, int n_sectors, int top_k,
                         std::vector<rr_place_match>& out)
{
    out.assign(top_k > 0 ? n_query * (size_t)top_k : 0, rr_place_match{});
    return rr_match_descriptors(ctx, query, (int)n_query, db, (int)n_db, n_rings, n_sectors, top_k, out.data(), nullptr, nullptr) == 0;
}

// object annotations (rr_object_note): n poses [n][7] in chunks of RR_MAX_BATCH through rr_simulate_batch_annotations -- one record per
// (frame, object), [n][n_objects], the skip counts [n] and, if asked for, the images [n][npx].  false: rr_last_error(ctx)
inline bool annotate_chunks(rr_ctx* ctx, const float* poses, size_t n, size_t n_objects, size_t npx, uint32_t extent_mask,
                            std::vector<rr_object_note>& notes, std::vector<uint32_t>& skipped, std::vector<uint8_t>* images)
{
    notes.assign(n * n_objects, rr_object_note{});
    skipped.assign(n, 0u);
    if (images) images->assign(n * npx, 0);
    for (size_t at = 0; at < n; at += RR_MAX_BATCH) {
        const size_t m = std::min<size_t>(RR_MAX_BATCH, n - at);
        if (rr_simulate_batch_annotations(ctx, poses + 7 * at, (int)m, extent_mask, images ? images->data() + at * npx : nullptr,
                                          notes.data() + at * n_objects, skipped.data() + at)) return false;
    }
    return true;
}

// likelihood field (rr_field_config, rr_field_rec): n clouds, each under its state (c, s, tx, ty: sensor frame into the map frame; states
// empty: the identity), rasterised into one occupancy grid (rr_rasterize_points) and transformed (rr_distance_field) into the field
// [height][width].  false: rr_last_error(ctx), or a states vector that is not [n][4]
inline bool build_field(rr_ctx* ctx, const std::vector<std::vector<rr_radar_point>>& clouds, const std::vector<double>& states, int n_angles,
                        const rr_field_config& cfg, std::vector<uint16_t>& field)
{
    const size_t n = clouds.size(), stride = (size_t)n_angles + 1;
    const size_t cells = cfg.width > 0 && cfg.height > 0 ? (size_t)cfg.width * (size_t)cfg.height : 0;
    field.assign(cells, 0);
    if (n == 0 || (!states.empty() && states.size() != 4 * n)) return false;
    size_t mp = 1;
    for (const auto& c : clouds) mp = std::max(mp, c.size());
    std::vector<rr_radar_point> pts(n * mp);
    std::vector<uint32_t> offs(n * stride, 0u);                       // only each frame's total is read
    for (size_t f = 0; f < n; f++) {
        std::copy(clouds[f].begin(), clouds[f].end(), pts.begin() + (std::ptrdiff_t)(f * mp));
        offs[f * stride + (size_t)n_angles] = (uint32_t)clouds[f].size();
    }
    std::vector<uint8_t> occ(cells, 0);
    if (rr_rasterize_points(ctx, pts.data(), offs.data(), (int)n, (int)mp, states.empty() ? nullptr : states.data(), &cfg, occ.data())) return false;
    return rr_distance_field(ctx, occ.data(), 1, &cfg, field.data()) == 0;
}

// one scan against n hypothesis states [n][4] f32 (c, s, tx, ty: the scan's sensor frame into the map frame) and a field (rr_score_poses):
// one record per hypothesis.  false: rr_last_error(ctx), or a states vector that is not [n][4], or a field that is not [height][width]
inline bool score_poses(rr_ctx* ctx, const std::vector<rr_radar_point>& scan, const std::vector<float>& states, const std::vector<uint16_t>& field,
                        const rr_field_config& cfg, std::vector<rr_field_rec>& out)
{
    out.assign(states.size() / 4, rr_field_rec{});
    if (states.empty() || states.size() % 4 || cfg.width < 1 || cfg.height < 1 || field.size() != (size_t)cfg.width * (size_t)cfg.height) return false;
    return rr_score_poses(ctx, scan.data(), (uint32_t)scan.size(), (int)scan.size(), states.data(), (int)(states.size() / 4), field.data(), &cfg,
                          out.data()) == 0;
}

// Correlative scan matching (rr_field_pyramid, rr_correlate_scan, host forms): one scan, n_rot anchor states [n_rot][4] f32 (c, s, tx, ty: the
// scan's sensor frame into the map frame at the centre of the window) and a field [height][width] -> the record of the node of smallest
// (sum_d2, index) over every rotation and every whole-cell offset of corr's window.  The field's min-pyramid is built for the call.
// false: rr_last_error(ctx), or a states vector that is not [n][4], or a field that is not [height][width], or levels outside 0..8
inline bool correlate_scan(rr_ctx* ctx, const std::vector<rr_radar_point>& scan, const std::vector<float>& rot, const std::vector<uint16_t>& field,
                           const rr_field_config& cfg, const rr_corr_config& corr, rr_corr_rec& out)
{
    out = rr_corr_rec{};
    const size_t cells = cfg.width > 0 && cfg.height > 0 ? (size_t)cfg.width * (size_t)cfg.height : 0;
    if (rot.empty() || rot.size() % 4 || cells == 0 || field.size() != cells || corr.levels < 0 || corr.levels > 8) return false;
    std::vector<uint16_t> pyramid(((size_t)corr.levels + 1) * cells);
    if (rr_field_pyramid(ctx, field.data(), &cfg, corr.levels, pyramid.data())) return false;
    return rr_correlate_scan(ctx, scan.data(), (uint32_t)scan.size(), (int)scan.size(), rot.data(), (int)(rot.size() / 4), pyramid.data(), &cfg, &corr,
                             &out) == 0;
}

// n clouds as the cloud calls take them: pts [n][mp] and offs [n][n_angles + 1], of which only each frame's total is read.  Returns mp, the
// longest cloud (1 at the least); 0 for no cloud or a cloud of more than 65536 points
inline size_t pack_clouds(const std::vector<std::vector<rr_radar_point>>& clouds, int n_angles, std::vector<rr_radar_point>& pts, std::vector<uint32_t>& offs)
{
    const size_t n = clouds.size(), stride = (size_t)n_angles + 1;
    size_t mp = 1;
    for (const auto& c : clouds) mp = std::max(mp, c.size());
    if (n == 0 || mp > 65536) return 0;
    pts.assign(n * mp, rr_radar_point{});
    offs.assign(n * stride, 0u);
    for (size_t f = 0; f < n; f++) {
        std::copy(clouds[f].begin(), clouds[f].end(), pts.begin() + (std::ptrdiff_t)(f * mp));
        offs[f * stride + (size_t)n_angles] = (uint32_t)clouds[f].size();
    }
    return mp;
}

// Oriented surface points (rr_surfel_config, rr_surfel; rr_surface_points, host form): n clouds -> per cloud its first
// min(kept, max_surfels) surface points in ascending cell order, and counts [n][2] = kept (the TRUE total), flags.
// false: rr_last_error(ctx), or no cloud, a cloud of more than 65536 points or a negative max_surfels
inline bool surface_points(rr_ctx* ctx, const std::vector<std::vector<rr_radar_point>>& clouds, int n_angles, const rr_surfel_config& cfg,
                           int max_surfels, std::vector<std::vector<rr_surfel>>& surfels, std::vector<uint32_t>& counts)
{
    surfels.clear(); counts.clear();
    const size_t n = clouds.size();
    std::vector<rr_radar_point> pts; std::vector<uint32_t> offs;
    const size_t mp = pack_clouds(clouds, n_angles, pts, offs);
    if (mp == 0 || max_surfels < 0) return false;
    const size_t cap = (size_t)max_surfels;
    std::vector<rr_surfel> recs(n * cap);
    counts.assign(2 * n, 0u);
    if (rr_surface_points(ctx, pts.data(), offs.data(), (int)n, (int)mp, &cfg, cap ? recs.data() : nullptr, max_surfels, counts.data()) != 0) {
        counts.clear();
        return false;
    }
    surfels.resize(n);
    for (size_t f = 0; f < n; f++)
        surfels[f].assign(recs.begin() + (std::ptrdiff_t)(f * cap), recs.begin() + (std::ptrdiff_t)(f * cap + std::min<size_t>(counts[2 * f], cap)));
    return true;
}

// Scan matching (rr_register_points / rr_register_surfels, host forms): n clouds registered against ONE target, a cloud by point-to-point ICP
// or surface points by point-to-line ICP, from the states `init` ([n][4] = c s tx ty per cloud) or, if it is empty, from the identity: one
// rr_icp_rec per cloud.  false: rr_last_error(ctx), or no cloud, a cloud or a target of more than 65536 records, or an init that is not [n][4]
inline int register_call(rr_ctx* ctx, const rr_radar_point* pts, const uint32_t* offs, int n, int mp, const rr_radar_point* tgt, uint32_t count,
                         const double* init, float gate, int iterations, rr_icp_rec* recs)
{
    return rr_register_points(ctx, pts, offs, n, mp, tgt, count, (int)count, init, gate, iterations, recs, nullptr);
}
inline int register_call(rr_ctx* ctx, const rr_radar_point* pts, const uint32_t* offs, int n, int mp, const rr_surfel* tgt, uint32_t count,
                         const double* init, float gate, int iterations, rr_icp_rec* recs)
{
    return rr_register_surfels(ctx, pts, offs, n, mp, tgt, count, (int)count, init, gate, iterations, recs, nullptr);
}
template <class Target>
inline bool register_clouds(rr_ctx* ctx, const std::vector<std::vector<rr_radar_point>>& clouds, int n_angles, const std::vector<Target>& target,
                            const std::vector<double>& init, float gate, int iterations, std::vector<rr_icp_rec>& recs)
{
    recs.clear();
    const size_t n = clouds.size();
    std::vector<rr_radar_point> pts; std::vector<uint32_t> offs;
    const size_t mp = pack_clouds(clouds, n_angles, pts, offs);
    if (mp == 0 || target.size() > 65536 || (!init.empty() && init.size() != 4 * n)) return false;
    recs.resize(n);
    if (register_call(ctx, pts.data(), offs.data(), (int)n, (int)mp, target.empty() ? nullptr : target.data(), (uint32_t)target.size(),
                      init.empty() ? nullptr : init.data(), gate, iterations, recs.data()) != 0) {
        recs.clear();
        return false;
    }
    return true;
}
inline bool register_surfels(rr_ctx* ctx, const std::vector<std::vector<rr_radar_point>>& clouds, int n_angles, const std::vector<rr_surfel>& target,
                             const std::vector<double>& init, float gate, int iterations, std::vector<rr_icp_rec>& recs)
{
    return register_clouds(ctx, clouds, n_angles, target, init, gate, iterations, recs);
}

// Pose-graph optimisation (rr_graph_edge, rr_graph_config, rr_graph_rec; rr_graph_plan and rr_optimize_graph, host forms): states [N][4] =
// (c, s, tx, ty) in and out, a fixed byte per node, the edges (a matcher's record with target i and source j is an edge as it comes) ->
// the optimised states and cfg.iterations + 1 records; the plan is built here.  false: rr_last_error(ctx), or states that are not [N][4]
// for N = fixed.size() in 1..2^20, more than 2^22 edges, or iterations outside 0..256 -- and the states keep their values
inline bool optimize_graph(rr_ctx* ctx, std::vector<double>& states, const std::vector<uint8_t>& fixed, const std::vector<rr_graph_edge>& edges,
                           const rr_graph_config& cfg, std::vector<rr_graph_rec>& recs)
{
    recs.clear();
    const size_t n = fixed.size(), ne = edges.size();
    if (n < 1 || n > ((size_t)1 << 20) || states.size() != 4 * n || ne > ((size_t)1 << 22) || cfg.iterations < 0 || cfg.iterations > 256) return false;
    std::vector<uint8_t> plan(rr_graph_plan_bytes((int)n, (int)ne));
    const rr_graph_edge* e = ne ? edges.data() : nullptr;
    if (plan.empty() || rr_graph_plan(ctx, e, (int)n, (int)ne, plan.data(), plan.size()) != 0) return false;
    std::vector<double> x(states);
    recs.resize((size_t)cfg.iterations + 1);
    if (rr_optimize_graph(ctx, x.data(), fixed.data(), e, (int)n, (int)ne, plan.data(), &cfg, recs.data(), nullptr) != 0) {
        recs.clear();
        return false;
    }
    states.swap(x);
    return true;
}

// map refinement: the nearest-cell table [height][width] of an occupancy map (occupied: >= threshold; rr_nearest_field), 0xFFFFFFFF where no
// occupied cell lies within cfg.max_dist.  false: rr_last_error(ctx), or a map that is not [height][width]
inline bool build_nearest(rr_ctx* ctx, const std::vector<uint8_t>& occ, int threshold, const rr_field_config& cfg, std::vector<uint32_t>& nearest)
{
    const size_t cells = cfg.width > 0 && cfg.height > 0 ? (size_t)cfg.width * (size_t)cfg.height : 0;
    nearest.assign(cells, 0xFFFFFFFFu);
    if (cells == 0 || occ.size() != cells) return false;
    return rr_nearest_field(ctx, occ.data(), threshold, &cfg, nearest.data()) == 0;
}

// Connected components (rr_label_components, host form): uint8 planes [n][height][width] -> per plane the kept components' records in
// ascending root order (comps[a]: the first min(kept, max_components)), counts [n][2] = kept, dropped, and as asked for (non-null) the
// label planes and the cleaned planes.  false: a plane buffer of the wrong size, or rr_last_error(ctx)
inline bool label_components(rr_ctx* ctx, const std::vector<uint8_t>& planes, int n_planes, const rr_components_config& cfg,
                             std::vector<std::vector<rr_component>>& comps, std::vector<uint32_t>& counts, std::vector<uint32_t>* labels,
                             std::vector<uint8_t>* clean)
{
    comps.clear(); counts.clear();
    const size_t npx = cfg.width > 0 && cfg.height > 0 ? (size_t)cfg.width * (size_t)cfg.height : 0;
    if (n_planes < 1 || npx == 0 || planes.size() != (size_t)n_planes * npx || cfg.max_components < 0) return false;
    const size_t n = (size_t)n_planes, cap = (size_t)cfg.max_components;
    std::vector<rr_component> recs(n * cap);
    counts.assign(2 * n, 0u);
    if (labels) labels->assign(n * npx, 0xFFFFFFFFu);
    if (clean) clean->assign(n * npx, 0);
    if (rr_label_components(ctx, planes.data(), n_planes, &cfg, labels ? labels->data() : nullptr, clean ? clean->data() : nullptr,
                            cap ? recs.data() : nullptr, counts.data()) != 0) return false;
    comps.resize(n);
    for (size_t a = 0; a < n; a++) comps[a].assign(recs.begin() + a * cap, recs.begin() + a * cap + std::min<size_t>(counts[2 * a], cap));
    return true;
}

// Windowed CFAR (rr_detect_window, host form) of ONE polar image of npx = n_cells * n_angles pixels: a count-only call sizes the points, a
// second call writes them (sorted by column, then bin) and, as asked for (non-null), the uint8 detection mask [n_cells][n_angles].
// false: rr_last_error(ctx)
inline bool detect_window(rr_ctx* ctx, const uint8_t* image, size_t npx, int n_angles, const rr_window_detect_config& cfg,
                          std::vector<rr_radar_point>& pts, std::vector<uint8_t>* mask)
{
    pts.clear();
    if (mask) mask->clear();
    std::vector<uint32_t> offs((size_t)n_angles + 1);
    if (rr_detect_window(ctx, image, 1, &cfg, nullptr, 0, offs.data(), nullptr) != 0) return false;      // count
    pts.resize(offs.back());
    if (mask) mask->assign(npx, 0);
    if (pts.empty() && !mask) return true;
    if (rr_detect_window(ctx, image, 1, &cfg, pts.empty() ? nullptr : pts.data(), (int)pts.size(), offs.data(), mask ? mask->data() : nullptr) != 0) {
        pts.clear();
        if (mask) mask->clear();
        return false;
    }
    return true;
}

// ... and ONE scan refined against it from n_hyp starting states on `stream`, every buffer the caller's and in HBM: d_init [n_hyp][4] f64
// (c, s, tx, ty: the scan's sensor frame into the map frame), d_recs [n_hyp] (rr_refine_poses_device: one launch, nothing comes home and
// nothing is waited for).  false: rr_last_error(ctx)
inline bool refine_poses(rr_ctx* ctx, const rr_radar_point* d_scan, const uint32_t* d_count, int max_points, const double* d_init, int n_hyp,
                         const uint32_t* d_nearest, const rr_field_config& cfg, int iterations, rr_icp_rec* d_recs, void* stream)
{
    return rr_refine_poses_device(ctx, d_scan, d_count, max_points, d_init, n_hyp, d_nearest, &cfg, iterations, d_recs, stream) == 0;
}

// the beam model (rr_beam_config), every buffer the caller's and in HBM, on `stream`: the map's field cast at n_hyp states -- d_states [n_hyp][4]
// f32 (c, s, tx, ty: the sensor frame into the map frame), d_dirs [n_angles][2] f32 -- into d_ranges uint16 [n_hyp][n_angles]
// (rr_cast_map_device), or scored against ONE profile d_first_bin uint16 [n_angles] of rr_scan_profile_device into d_recs [n_hyp]
// (rr_score_beams_device): one launch each, nothing comes home and nothing is waited for.  false: rr_last_error(ctx)
inline bool cast_map(rr_ctx* ctx, const float* d_states, int n_hyp, const float* d_dirs, const uint16_t* d_field, const rr_field_config& cfg,
                     const rr_beam_config& beam, uint16_t* d_ranges, void* stream)
{
    return rr_cast_map_device(ctx, d_states, n_hyp, d_dirs, d_field, &cfg, &beam, d_ranges, stream) == 0;
}
inline bool score_beams(rr_ctx* ctx, const uint16_t* d_first_bin, const float* d_states, int n_hyp, const float* d_dirs, const uint16_t* d_field,
                        const rr_field_config& cfg, const rr_beam_config& beam, rr_beam_rec* d_recs, void* stream)
{
    return rr_score_beams_device(ctx, d_first_bin, d_states, n_hyp, d_dirs, d_field, &cfg, &beam, d_recs, stream) == 0;
}

// occupancy mapping (rr_occupancy_config): n clouds, each sorted by column then bin as rr_detect writes them and under its state (states
// empty: the identity), fused into the int32 evidence [height][width] -- accumulated into what `evidence` holds if it has the grid's size,
// else into zeros (rr_occupancy_update) -- and clamped into the byte map (rr_occupancy_map).  The offsets of each cloud are rebuilt from
// its points' columns.  false: rr_last_error(ctx), or a states vector that is not [n][4], or a cloud that is not sorted by column
inline bool sorted_by_column(const std::vector<rr_radar_point>& cloud, int n_angles)
{
    uint32_t last = 0;
    for (const rr_radar_point& p : cloud) {
        if (p.column >= (uint32_t)n_angles || p.column < last) return false;
        last = p.column;
    }
    return true;
}
inline bool build_occupancy(rr_ctx* ctx, const std::vector<std::vector<rr_radar_point>>& clouds, const std::vector<double>& states, int n_angles,
                            const rr_field_config& cfg, const rr_occupancy_config& occ_cfg, std::vector<int32_t>& evidence, std::vector<uint8_t>& map)
{
    const size_t n = clouds.size(), stride = (size_t)n_angles + 1;
    const size_t cells = cfg.width > 0 && cfg.height > 0 ? (size_t)cfg.width * (size_t)cfg.height : 0;
    if (evidence.size() != cells) evidence.assign(cells, 0);
    map.assign(cells, 0);
    if (n == 0 || (!states.empty() && states.size() != 4 * n)) return false;
    size_t mp = 1;
    for (const auto& c : clouds) mp = std::max(mp, c.size());
    std::vector<rr_radar_point> pts(n * mp);
    std::vector<uint32_t> offs(n * stride, 0u);
    for (size_t f = 0; f < n; f++) {
        std::copy(clouds[f].begin(), clouds[f].end(), pts.begin() + (std::ptrdiff_t)(f * mp));
        if (!sorted_by_column(clouds[f], n_angles)) return false;
        uint32_t* o = offs.data() + f * stride;
        for (const rr_radar_point& p : clouds[f]) o[p.column + 1]++;   // counts, one slot up ...
        for (size_t a = 0; a < (size_t)n_angles; a++) o[a + 1] += o[a];   // ... summed into the exclusive prefix, the total last
    }
    if (rr_occupancy_update(ctx, pts.data(), offs.data(), (int)n, (int)mp, states.empty() ? nullptr : states.data(), &cfg, &occ_cfg, evidence.data()))
        return false;
    return rr_occupancy_map(ctx, evidence.data(), &cfg, map.data()) == 0;
}

// one particle filter step on `stream`, every buffer the caller's and in HBM (rr_filter_config, rr_filter_summary): the particles d_states_in
// [n][4] f32 scored against the field (rr_score_poses_device -> d_recs [n]), the records weighed through d_table and resampled
// (rr_filter_resample_device -> d_cum [n], d_ancestors [n], d_summary), the survivors moved by the increment (Dc, Ds, dx, dy) plus the
// config's diffusion into d_states_out [n][4] (rr_filter_move_device; resample false: every particle is kept, the move runs without
// ancestors).  Only the 32-byte summary comes home.  false: rr_last_error(ctx)
inline bool filter_step(rr_ctx* ctx, const rr_radar_point* d_scan, const uint32_t* d_count, int max_points, const float* d_states_in, int n,
                        const uint16_t* d_field, const rr_field_config& cfg, const uint16_t* d_table, const rr_filter_config& fcfg,
                        const float (&increment)[4], bool resample, rr_field_rec* d_recs, uint64_t* d_cum, uint32_t* d_ancestors,
                        float* d_states_out, rr_filter_summary* d_summary, void* stream, rr_filter_summary& summary)
{
    summary = rr_filter_summary{};
    if (rr_score_poses_device(ctx, d_scan, d_count, max_points, d_states_in, n, d_field, &cfg, d_recs, stream)) return false;
    if (rr_filter_resample_device(ctx, d_recs, n, d_table, n, &fcfg, d_cum, d_ancestors, d_summary, stream)) return false;
    if (rr_filter_move_device(ctx, d_states_in, n, resample ? d_ancestors : nullptr, n, increment[0], increment[1], increment[2], increment[3], &fcfg,
                              d_states_out, stream))
        return false;
    if (rr_copy_to_host_async(ctx, d_summary, &summary, sizeof(summary), stream)) return false;
    return rr_synchronize(ctx, stream) == 0;
}

}  // namespace radarays_ros_amd::marshal
