// RadarHIP.hpp -- C++ host side above the C ABI, mirroring the reference's backend interface.
//
// Reference (C++):  include/radarays_ros/Radar.hpp:34-105   abstract `Radar` (the seam:
//                   `virtual sensor_msgs::ImagePtr simulate(ros::Time) = 0`, :64)
//                   src/radarays_ros/Radar.cpp:10-41,188-226 ctor constants, updateDynCfg, loadParams
//                   include/radarays_ros/RadarCPU.hpp:21-28  a concrete backend
// This header keeps the same member names, argument meaning and error behaviour, minus the
// ROS / OpenCV / rmagine types this image does not have: TF lookup becomes updateTsm(pose),
// sensor_msgs::Image becomes the plain `Image` struct with the same fields, rm::Transform
// becomes float[7] (quaternion xyzw + translation).  INTEGRATION.md shows the ROS-typed twin.
// What the two classes do alike -- config copy, materials, beam draw, chunked batches, parameter sets -- is marshal.hpp,
// which both include: the marshalling the ROS-typed adapter ships is the one the GPU demo executes through this class.
// Here: the `Radar` base, the dirty flags, `Image`s, detect / detectWindow / toCartesian and how errors are reported.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "marshal.hpp"

namespace radarays_ros_amd {

// msg/RadarMaterial.msg, msg/RadarModel.msg, msg/RadarParams.msg
struct RadarMaterial { float velocity = 0.3f, ambient = 1.0f, diffuse = 0.0f, specular = 1.0f; };
struct RadarModel { float beam_width = 8.0f * (float)M_PI / 180.0f; uint32_t n_samples = 200; uint32_t n_reflections = 2; };
struct RadarParams { std::vector<RadarMaterial> materials; RadarModel model; };

// cfg/RadarModel.cfg:11-85 (the fields the hot path reads; same names and defaults)
struct RadarModelConfig {
    double beam_width = 8.0, resolution = 0.0438;
    int n_cells = 3424, n_samples = 10, beam_sample_dist = 2;
    double beam_sample_dist_normal_p_in_cone = 0.8;
    int n_reflections = 4;
    double energy_max = 0.5, signal_max = 120.0;
    int signal_denoising = 1;
    int signal_denoising_triangular_width = 50; double signal_denoising_triangular_mode = 0.35;
    int signal_denoising_gaussian_width = 50;   double signal_denoising_gaussian_mode = 0.5;
    int signal_denoising_mb_width = 50;         double signal_denoising_mb_mode = 0.4;
    int ambient_noise = 2;
    double ambient_noise_at_signal_0 = 0.3, ambient_noise_at_signal_1 = 0.03;
    double ambient_noise_energy_max = 0.5, ambient_noise_energy_min = 0.1, ambient_noise_energy_loss = 0.05;
    int scroll_image = 0;
    double multipath_threshold = 0.5;
    bool record_multi_reflection = true, record_multi_path = false, include_motion = true;
};

// sensor_msgs/Image as RadarCPU.cpp:555-561 fills it
struct Image {
    double stamp = 0.0; std::string frame_id;
    uint32_t height = 0, width = 0, step = 0; std::string encoding = "mono8";
    std::vector<uint8_t> data;
};
using ImagePtr = std::shared_ptr<Image>;

class Radar {   // Radar.hpp:34
public:
    Radar(std::string map_frame, std::string sensor_frame)
    : m_map_frame(std::move(map_frame)), m_sensor_frame(std::move(sensor_frame)) {}   // Radar.cpp:10-41
    virtual ~Radar() = default;

    void loadParams(const std::vector<RadarMaterial>& materials, const std::vector<int>& object_materials,
                    int material_id_air)   // Radar.cpp:220-226 (ROS parameter server -> arguments)
    { m_params.materials = materials; m_object_materials = object_materials; m_material_id_air = material_id_air; m_dirty_mat = true; }
    RadarParams getParams() const { return m_params; }
    void setParams(const RadarParams& p) { m_params = p; m_dirty_mat = true; m_dirty_cfg = true; }

    void updateDynCfg(const RadarModelConfig& config)   // Radar.cpp:188-218
    {
        if (config.beam_sample_dist != m_cfg.beam_sample_dist || std::abs(config.beam_width - m_cfg.beam_width) > 0.001 ||
            config.n_samples != m_cfg.n_samples ||
            std::abs(config.beam_sample_dist_normal_p_in_cone - m_cfg.beam_sample_dist_normal_p_in_cone) > 0.001)
            m_resample = true;
        m_params.model.beam_width = (float)(config.beam_width * M_PI / 180.0);
        m_params.model.n_samples = (uint32_t)config.n_samples;
        m_params.model.n_reflections = (uint32_t)config.n_reflections;
        m_cfg = config; m_dirty_cfg = true;
    }
    bool updateTsm() const { return has_last; }                 // Radar.cpp:80-132: TF lookup, last pose as fallback
    bool updateTsm(const float pose_qxyzw_t[7])
    {
        for (int k = 0; k < 7; k++) if (!std::isfinite(pose_qxyzw_t[k])) return has_last;
        for (int k = 0; k < 7; k++) Tsm_last[k] = pose_qxyzw_t[k];
        has_last = true; return true;
    }
    virtual ImagePtr simulate(double stamp) = 0;                 // Radar.hpp:64

protected:
    float Tsm_last[7] = { 0, 0, 0, 1, 0, 0, 0 }; bool has_last = false;
    std::string m_map_frame, m_sensor_frame;
    RadarParams m_params;
    RadarModelConfig m_cfg;
    int m_material_id_air = 0;                 // Radar.cpp:23
    std::vector<int> m_object_materials;
    float m_wave_energy_threshold = 0.001f;    // Radar.cpp:24
    std::vector<float> m_waves_start;          // beam sample directions [n][3]
    bool m_resample = true;                    // Radar.cpp:25
    bool m_dirty_cfg = true, m_dirty_mat = true;
};

class RadarHIP : public Radar {   // sibling of RadarCPU (RadarCPU.hpp:16-37)
public:
    // One backend object per process like the reference (radar_simulator.cpp:145-176); `devices` lists the GPUs
    // of this node it fans out over (rr_multi: azimuth blocks, one RCCL collective per frame).
    RadarHIP(std::string map_frame, std::string sensor_frame, const std::vector<float>& verts,
             const std::vector<uint32_t>& faces, const std::vector<uint32_t>& face_object, const std::vector<int>& devices,
             bool build_on_gpu = false /* rr_set_mesh_gpu: the map loads in 0.35 s instead of 1.9 s at 10M triangles, frames take 1.2x as long */)
    : Radar(std::move(map_frame), std::move(sensor_frame))
    {
        m_multi = rr_create_multi(devices.data(), (int)devices.size());
        if (!m_multi) throw std::runtime_error(rr_multi_last_error(nullptr));
        m_ctx = rr_multi_ctx(m_multi, 0);
        if ((build_on_gpu ? rr_multi_set_mesh_gpu : rr_multi_set_mesh)(m_multi, verts.data(), verts.size() / 3, faces.data(), faces.size() / 3,
                                                                        face_object.empty() ? nullptr : face_object.data())) {
            std::string e = rr_multi_last_error(m_multi); rr_destroy_multi(m_multi); throw std::runtime_error(e);
        }
        for (uint32_t o : face_object) m_n_objects = std::max<size_t>(m_n_objects, (size_t)o + 1);
    }
    RadarHIP(std::string map_frame, std::string sensor_frame, const std::vector<float>& verts,
             const std::vector<uint32_t>& faces, const std::vector<uint32_t>& face_object, int device = 0)
    : RadarHIP(std::move(map_frame), std::move(sensor_frame), verts, faces, face_object, std::vector<int>{ device }) {}
    ~RadarHIP() override { rr_destroy_multi(m_multi); }
    RadarHIP(const RadarHIP&) = delete;
    RadarHIP& operator=(const RadarHIP&) = delete;

    // m_waves_start: RadarCPU::simulate draws them with sample_cone_local whenever m_resample is set (RadarCPU.cpp:136-145),
    // seeding from std::random_device.  push() does the same (rr_sample_cone_local); setBeamSeed() makes the draw
    // reproducible, setBeamSamples() injects directions from any other generator -- [n][3], local frame -- until the next
    // dynamic reconfigure of the beam asks for a re-draw again
    void setBeamSeed(uint32_t seed) { m_beam_seed = seed; m_have_seed = true; }
    void setBeamSamples(const std::vector<float>& dirs) { m_waves_start = dirs; m_resample = false; m_push_beams = true; }
    const std::vector<float>& beamSamples() const { return m_waves_start; }
    void setNoiseOffsets(const std::vector<float>& rnd) { rr_multi_set_noise_offsets(m_multi, rnd.data(), rnd.size()); }
    // include_motion (cfg/RadarModel.cfg:85, RadarCPU.cpp:190-196): the reference looks Tsm up once PER AZIMUTH while
    // the antenna turns; the TF lookups of one sweep arrive here as [n_angles][7] and are used while
    // m_cfg.include_motion is set (an empty vector: one pose per frame again)
    void setMotionPoses(const std::vector<float>& poses_per_azimuth) { m_motion = poses_per_azimuth; m_push_motion = true; }

    ImagePtr simulate(double stamp) override   // RadarCPU.cpp:30-564
    {
        ImagePtr msg;
        if (!updateTsm()) {
            std::cout << "Couldn't get Transform between sensor and map. Skipping..." << std::endl;   // RadarCPU.cpp:131
            return msg;
        }
        if (!push()) return msg;
        msg = image(nullptr, stamp);
        if (rr_multi_device_count(m_multi) > 1) {
            if (rr_multi_simulate(m_multi, Tsm_last, msg->data.data())) { mfail(); return {}; }
        } else if (rr_simulate(m_ctx, Tsm_last, 0, m_n_angles, msg->data.data(), nullptr, &m_stats)) return fail();
        return msg;
    }
    // What the image is made of (rr_simulate_provenance, include/radarays_mi355.h), on device 0: the frame at the current Tsm and,
    // per pixel, the info word (object | pass << 24 | kind << 28) and the face of the echo with the largest single term in that
    // range bin (RR_LABEL_NONE: none); per azimuth its ordered echo stream, rows of `echo_stride` records (0: no stream), and the
    // true counts.  A ghost mask is pass > 0, a semantic mask is object -> material.  Null on error (lastError()).
    struct Provenance { ImagePtr image; std::vector<uint32_t> labels, faces, echo_counts; std::vector<rr_echo_src> echoes; size_t echo_stride = 0; };
    std::shared_ptr<Provenance> simulateProvenance(double stamp, size_t echo_stride = 0)
    {
        if (!updateTsm()) {
            std::cout << "Couldn't get Transform between sensor and map. Skipping..." << std::endl;
            return {};
        }
        if (!push()) return {};
        auto out = std::make_shared<Provenance>();
        out->image = image(nullptr, stamp);
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        out->labels.assign(npx, RR_LABEL_NONE); out->faces.assign(npx, RR_LABEL_NONE);
        out->echo_counts.assign((size_t)m_n_angles, 0u);
        out->echoes.resize((size_t)m_n_angles * echo_stride); out->echo_stride = echo_stride;
        if (rr_simulate_provenance(m_ctx, Tsm_last, out->image->data.data(), out->labels.data(), out->faces.data(),
                                   echo_stride ? out->echoes.data() : nullptr, echo_stride, out->echo_counts.data())) { fail(); return {}; }
        return out;
    }
    // By which route the waves travelled (rr_simulate_paths, include/radarays_mi355.h), on device 0: the frame at the current Tsm and,
    // per azimuth, its list of ray-cast waves (misses included), rows of `wave_stride` records (0: one run first to learn the counts),
    // the true counts and the waves per pass.  map_frame: o / d in the map frame.  Null on error (lastError()).
    struct Paths { ImagePtr image; std::vector<rr_wave_rec> waves; std::vector<uint32_t> wave_counts, pass_counts; size_t wave_stride = 0; };
    std::shared_ptr<Paths> simulatePaths(double stamp, size_t wave_stride = 0, bool map_frame = false)
    {
        if (!updateTsm()) {
            std::cout << "Couldn't get Transform between sensor and map. Skipping..." << std::endl;
            return {};
        }
        if (!push()) return {};
        auto out = std::make_shared<Paths>();
        out->image = image(nullptr, stamp);
        out->wave_counts.assign((size_t)m_n_angles, 0u);
        out->pass_counts.assign((size_t)m_n_angles * RR_WAVES_MAX_PASSES, 0u);
        const unsigned flags = map_frame ? RR_WAVES_MAP_FRAME : 0u;
        if (wave_stride == 0) {
            if (rr_simulate_paths(m_ctx, Tsm_last, out->image->data.data(), nullptr, 0, out->wave_counts.data(), nullptr, flags)) { fail(); return {}; }
            for (uint32_t n : out->wave_counts) wave_stride = std::max(wave_stride, (size_t)n);
            wave_stride = std::max<size_t>(wave_stride, 1);
        }
        out->waves.resize((size_t)m_n_angles * wave_stride); out->wave_stride = wave_stride;
        if (rr_simulate_paths(m_ctx, Tsm_last, out->image->data.data(), out->waves.data(), wave_stride, out->wave_counts.data(),
                              out->pass_counts.data(), flags)) { fail(); return {}; }
        return out;
    }
    // A ghost's route: the wave of ONE azimuth's list (its first n records) that owns echo k of the azimuth's echo stream, walked back
    // along `parent` to the emitted beam -> the indices of the chain's waves, beam first (empty: no record owns echo k, or a parent
    // lies beyond n -- a truncated row -- or the chain is longer than RR_WAVES_MAX_PASSES).  The polyline is records[i].o of the first, then o + range * d of every wave of the chain.
    static std::vector<int32_t> pathToEcho(const rr_wave_rec* records, size_t n, int32_t k)
    {
        std::vector<int32_t> chain;
        for (size_t i = 0; i < n && chain.empty(); i++) {
            const int32_t owned = (int32_t)((records[i].info >> 30) & 1u) + (int32_t)(records[i].info >> 31);
            if (records[i].echo >= 0 && records[i].echo <= k && k < records[i].echo + owned) chain.push_back((int32_t)i);
        }
        while (!chain.empty() && records[chain.back()].parent >= 0) {
            const int32_t p = records[chain.back()].parent;
            if ((size_t)p >= n || chain.size() >= RR_WAVES_MAX_PASSES) return {};      // one wave per pass: no longer chain is a wave list's
            chain.push_back(p);
        }
        std::reverse(chain.begin(), chain.end());
        return chain;
    }
    // The frame as an FMCW sweep sees a moving scene (rr_simulate_doppler, include/radarays_mi355.h), on device 0: the image of the
    // shifted echo stream at the current Tsm and, per azimuth, every echo's range rate and shifted cell (-1: dropped), rows of
    // `echo_stride` entries (0: one run first to learn the counts), the true counts and the velocity image (NaN: no echo reaches the
    // bin).  sensor_vel: map frame, m/s (null: 0); gain: kappa in seconds; the objects' twists: rr_set_object_twists.  Null on error.
    struct Doppler { ImagePtr image; std::vector<float> echo_vel, vel_image; std::vector<int32_t> echo_cells; std::vector<uint32_t> echo_counts; size_t echo_stride = 0; };
    std::shared_ptr<Doppler> simulateDoppler(double stamp, const float* sensor_vel, float gain, size_t echo_stride = 0)
    {
        if (!updateTsm()) {
            std::cout << "Couldn't get Transform between sensor and map. Skipping..." << std::endl;
            return {};
        }
        if (!push()) return {};
        auto out = std::make_shared<Doppler>();
        out->image = image(nullptr, stamp);
        out->echo_counts.assign((size_t)m_n_angles, 0u);
        if (echo_stride == 0) {
            if (rr_simulate_doppler(m_ctx, Tsm_last, sensor_vel, gain, out->image->data.data(), nullptr, nullptr, 0, out->echo_counts.data(), nullptr, nullptr)) { fail(); return {}; }
            for (uint32_t n : out->echo_counts) echo_stride = std::max(echo_stride, (size_t)n);
            echo_stride = std::max<size_t>(echo_stride, 1);
        }
        out->echo_vel.assign((size_t)m_n_angles * echo_stride, 0.0f); out->echo_cells.assign((size_t)m_n_angles * echo_stride, -1);
        out->vel_image.assign(out->image->data.size(), 0.0f); out->echo_stride = echo_stride;
        if (rr_simulate_doppler(m_ctx, Tsm_last, sensor_vel, gain, out->image->data.data(), nullptr, out->echo_vel.data(), echo_stride, out->echo_counts.data(),
                                out->echo_cells.data(), out->vel_image.data())) { fail(); return {}; }
        return out;
    }
    // Offline generation (the twin of integration/src/radarays_ros/RadarHIP.cpp: simulateBatch / simulateSweeps): one image
    // per pose [n][7], up to RR_MAX_BATCH poses per set of launches; with per-azimuth pose tables (include_motion,
    // RadarCPU.cpp:190-196) sweeps = [n][n_angles][7], one table per frame (rr_multi_set_motion_poses)
    std::vector<ImagePtr> simulateBatch(const std::vector<float>& poses, double stamp) { return batch(poses, false, stamp); }
    std::vector<ImagePtr> simulateSweeps(const std::vector<float>& sweeps, double stamp) { return batch(sweeps, true, stamp); }

    // The gen_radar_image action of the optimisation loop (action/GenRadarImage.action,
    // scripts/radaray_opti.py:170-200), batched: one image per material table, same pose, one call.
    std::vector<ImagePtr> simulateMaterialSets(const std::vector<std::vector<RadarMaterial>>& sets, double stamp)
    {
        std::vector<ImagePtr> out;
        if (!updateTsm()) {
            std::cout << "Couldn't get Transform between sensor and map. Skipping..." << std::endl;
            return out;
        }
        if (!push()) return out;
        const size_t n_mat = m_params.materials.size();
        std::vector<rr_material> flat;
        for (const auto& set : sets) {
            if (set.size() != n_mat) { m_err = "every material set needs as many entries as loadParams() gave"; return out; }
            marshal::append_materials(flat, set.begin(), set.end());
        }
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        std::vector<uint8_t> px(sets.size() * npx);
        if (rr_simulate_material_sets(m_ctx, Tsm_last, flat.data(), (int)sets.size(), n_mat, px.data())) { fail(); return out; }
        for (size_t k = 0; k < sets.size(); k++) out.push_back(image(&px[k * npx], stamp));
        return out;
    }
    // The same action with the optimiser's WHOLE parameter vector (scripts/radaray_opti.py:36-113: model.beam_width,
    // model.n_reflections, the material values): one RadarParams per evaluation, one call for all of them
    // (rr_simulate_param_sets: sets with the same beam_width share pass 0, sets with fewer passes stop early).  The beam of
    // a set is drawn like push() draws it -- with the very seed push() used for the current beam, so equal widths give equal
    // directions and sets that differ only in beam_width share their variates;
    // model.n_samples must be the current one.  `real` given: the objective values of radaray_opti.py:196 come back
    // (PSNR against the real image, skimage's formula; the optimiser minimises its negative) and, with want_images false,
    // no image leaves the GPU.
    bool simulateParamSets(const std::vector<RadarParams>& sets, double stamp, std::vector<ImagePtr>* images,
                           const Image* real = nullptr, std::vector<double>* psnr = nullptr)
    {
        if (!updateTsm()) { std::cout << "Couldn't get Transform between sensor and map. Skipping..." << std::endl; return false; }
        if (!push()) return false;
        const size_t n_mat = m_params.materials.size(), nb = m_params.model.n_samples;
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        if (real && (real->data.size() != npx || !psnr)) { m_err = "the real image must be n_cells x n_angles mono8 (and psnr given)"; return false; }
        // any number of sets goes on to the library (the ROS-typed adapter refuses more than RR_MAX_BATCH itself); the seed is
        // the one push() drew the CURRENT beam with
        marshal::ParamSetBatch b;
        if (!b.build(sets, [](const RadarParams& p) -> const auto& { return p.materials; }, n_mat, nb,
                     m_params.model.beam_width, m_beam_seed, m_cfg.beam_sample_dist, (float)m_cfg.beam_sample_dist_normal_p_in_cone, m_err)) return false;
        std::vector<uint8_t> px(images ? sets.size() * npx : 0);
        if (psnr) psnr->assign(sets.size(), 0.0);
        if (!b.run(m_ctx, Tsm_last, n_mat, images ? px.data() : nullptr, real ? real->data.data() : nullptr, real ? psnr->data() : nullptr)) { fail(); return false; }
        if (images) {
            images->clear();
            for (size_t k = 0; k < sets.size(); k++) images->push_back(image(&px[k * npx], stamp));
        }
        return true;
    }
    // ... and with any of the metrics the reference's script imports as the objective (SSIM, PSNR, NMI, VoI, mutual information:
    // rr_image_metrics, include/radarays_mi355.h): one record per set against `real`; `images` may be null
    bool simulateParamSetsMetrics(const std::vector<RadarParams>& sets, double stamp, std::vector<ImagePtr>* images, const Image& real,
                                  uint32_t which, int win_size, std::vector<rr_image_metrics>* out)
    {
        if (!updateTsm()) { std::cout << "Couldn't get Transform between sensor and map. Skipping..." << std::endl; return false; }
        if (!push()) return false;
        const size_t n_mat = m_params.materials.size(), nb = m_params.model.n_samples;
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        if (real.data.size() != npx || !out) { m_err = "the real image must be n_cells x n_angles mono8 (and out given)"; return false; }
        marshal::ParamSetBatch b;
        if (!b.build(sets, [](const RadarParams& p) -> const auto& { return p.materials; }, n_mat, nb,
                     m_params.model.beam_width, m_beam_seed, m_cfg.beam_sample_dist, (float)m_cfg.beam_sample_dist_normal_p_in_cone, m_err)) return false;
        std::vector<uint8_t> px(images ? sets.size() * npx : 0);
        out->assign(sets.size(), rr_image_metrics{});
        if (!b.run_metrics(m_ctx, Tsm_last, n_mat, images ? px.data() : nullptr, real.data.data(), which, win_size, out->data())) { fail(); return false; }
        if (images) {
            images->clear();
            for (size_t k = 0; k < sets.size(); k++) images->push_back(image(&px[k * npx], stamp));
        }
        return true;
    }
    // The "real to sim gap" (launch/tests/eval_real_to_sim.launch): mono8 polar images of this model's shape against ONE
    // real image, one record per image (fields of metrics not in `which` are 0).  Empty on error (lastError()).
    std::vector<rr_image_metrics> compareImages(const std::vector<ImagePtr>& images, const Image& real,
                                                uint32_t which = RR_METRIC_PSNR | RR_METRIC_SSIM | RR_METRIC_INFO, int win_size = 7)
    {
        std::vector<rr_image_metrics> out;
        if (images.empty() || !push()) return out;
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        bool ok = real.height == (uint32_t)m_cfg.n_cells && real.width == (uint32_t)m_n_angles && real.data.size() == npx;
        for (const ImagePtr& im : images) ok = ok && im && im->height == real.height && im->width == real.width && im->data.size() == npx;
        if (!ok) { m_err = "compareImages: every image must be n_cells x n_angles mono8"; std::cout << "[RadarHIP] " << m_err << std::endl; return out; }
        if (!marshal::compare_images(m_ctx, images.size(), npx, [&](size_t k) { return images[k]->data.data(); }, real.data.data(), which, win_size, out)) {
            fail(); out.clear();
        }
        return out;
    }
    // Azimuth registration (rr_align_record, include/radarays_mi355.h): the circular shift along the azimuth axis -- the amount
    // to add to scroll_image -- at which each image matches `real` best over the cell window [cell_begin, cell_end) (cell_end < 0:
    // n_cells), with the exact SSE, PSNR and NCC there; `curve` (or null) receives xcorr at every shift, [n][n_angles].  Empty on error.
    std::vector<rr_align_record> alignImages(const std::vector<ImagePtr>& images, const Image& real, int cell_begin = 0, int cell_end = -1,
                                             std::vector<int64_t>* curve = nullptr)
    {
        std::vector<rr_align_record> out;
        if (images.empty() || !push()) return out;
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        bool ok = real.height == (uint32_t)m_cfg.n_cells && real.width == (uint32_t)m_n_angles && real.data.size() == npx;
        for (const ImagePtr& im : images) ok = ok && im && im->height == real.height && im->width == real.width && im->data.size() == npx;
        if (!ok) { m_err = "alignImages: every image must be n_cells x n_angles mono8"; std::cout << "[RadarHIP] " << m_err << std::endl; return out; }
        if (!marshal::align_images(m_ctx, images.size(), npx, (size_t)m_n_angles, [&](size_t k) { return images[k]->data.data(); }, real.data.data(),
                                   cell_begin, cell_end < 0 ? m_cfg.n_cells : cell_end, out, curve)) {
            fail(); out.clear();
        }
        return out;
    }
    // Translation registration (rr_shift_record, include/radarays_mi355.h): the images and `real` made Cartesian (width x width,
    // pixel_size m/pixel) and compared over -max_shift..max_shift pixels on both axes; (dy, dx) is where an image's content is found in
    // `real`, with the exact SSE, PSNR and NCC there.  `correction` (or null) receives what to add to each image's pose in the
    // sensor's own axes, metres [n][2] = (forward, left).  Empty on error.
    std::vector<rr_shift_record> registerTranslation(const std::vector<ImagePtr>& images, const Image& real, int width, float pixel_size, int max_shift,
                                                     bool bilinear = true, std::vector<double>* correction = nullptr)
    {
        std::vector<rr_shift_record> out;
        if (images.empty() || !push()) return out;
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        bool ok = real.height == (uint32_t)m_cfg.n_cells && real.width == (uint32_t)m_n_angles && real.data.size() == npx;
        for (const ImagePtr& im : images) ok = ok && im && im->height == real.height && im->width == real.width && im->data.size() == npx;
        if (!ok) { m_err = "registerTranslation: every image must be n_cells x n_angles mono8"; std::cout << "[RadarHIP] " << m_err << std::endl; return out; }
        if (!marshal::register_translation(m_ctx, images.size(), npx, [&](size_t k) { return images[k]->data.data(); }, real.data.data(),
                                           width, pixel_size, max_shift, bilinear, out, correction)) {
            fail(); out.clear();
        }
        return out;
    }
    // Place recognition (rr_place_config, rr_place_match, include/radarays_mi355.h): the images' ring/sector descriptors,
    // [n][n_rings][n_sectors] bytes; a yaw of the sensor is a circular shift of a descriptor's sectors.  Empty on error.
    std::vector<uint8_t> describeImages(const std::vector<ImagePtr>& images, const rr_place_config& cfg)
    {
        std::vector<uint8_t> desc;
        if (images.empty() || !push()) return desc;
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        bool ok = true;
        for (const ImagePtr& im : images) ok = ok && im && im->height == (uint32_t)m_cfg.n_cells && im->width == (uint32_t)m_n_angles && im->data.size() == npx;
        if (!ok) { m_err = "describeImages: every image must be n_cells x n_angles mono8"; std::cout << "[RadarHIP] " << m_err << std::endl; return desc; }
        if (!marshal::describe(m_ctx, images.size(), npx, [&](size_t k) { return images[k]->data.data(); }, cfg, desc)) { fail(); desc.clear(); }
        return desc;
    }
    // One real image looked up in a database of descriptors (describeImages' layout, n_db of them): the top_k candidates by
    // (sse, index); a hit's pose is the database pose turned by +shift * (n_angles / n_sectors) * theta_inc about the sensor's z
    // axis (exact only when n_sectors divides n_angles).  Empty on error.
    std::vector<rr_place_match> localize(const Image& real, const std::vector<uint8_t>& database, size_t n_db, const rr_place_config& cfg, int top_k)
    {
        std::vector<rr_place_match> out;
        if (!push()) return out;
        const size_t npx = (size_t)m_cfg.n_cells * m_n_angles;
        const size_t K = cfg.n_rings > 0 && cfg.n_sectors > 0 ? (size_t)cfg.n_rings * (size_t)cfg.n_sectors : 0;
        if (real.height != (uint32_t)m_cfg.n_cells || real.width != (uint32_t)m_n_angles || real.data.size() != npx || database.size() != n_db * K) {
            m_err = "localize: the image must be n_cells x n_angles mono8 and the database n_db descriptors"; std::cout << "[RadarHIP] " << m_err << std::endl;
            return out;
        }
        std::vector<uint8_t> q;
        if (!marshal::describe(m_ctx, 1, npx, [&](size_t) { return real.data.data(); }, cfg, q) ||
            !marshal::match_places(m_ctx, q.data(), 1, database.data(), n_db, cfg.n_rings, cfg.n_sectors, top_k, out)) { fail(); out.clear(); }
        return out;
    }
    // Ground truth per object (rr_object_note, include/radarays_mi355.h), on device 0: for poses [n][7] one record per (frame, object),
    // [n][objectCount()] -- pixel counts by class, range / azimuth / Cartesian extent, peak and summed intensity of the pixels whose class
    // is in `extent_mask` (RR_NOTE_DIRECT | RR_NOTE_GHOST | RR_NOTE_MULTIPATH).  The label planes never leave the GPU; `images` (or null)
    // receives the frames.  Null on error (lastError()).
    struct Annotations { std::vector<rr_object_note> notes; std::vector<uint32_t> skipped; std::vector<ImagePtr> images; size_t n_objects = 0; };
    size_t objectCount() const { return m_n_objects; }
    std::shared_ptr<Annotations> simulateAnnotations(const std::vector<float>& poses, double stamp, uint32_t extent_mask = RR_NOTE_DIRECT,
                                                     bool want_images = false)
    {
        if (!push()) return {};
        if (poses.empty() || poses.size() % 7) { m_err = "poses must be [n][7]"; return {}; }
        const size_t n = poses.size() / 7, npx = (size_t)m_cfg.n_cells * m_n_angles;
        auto out = std::make_shared<Annotations>();
        out->n_objects = m_n_objects;
        std::vector<uint8_t> px;
        // one pose per frame, as in simulateBatch: a per-azimuth table that simulate() installed would stand in for every pose given here
        if (rr_multi_set_motion_poses(m_multi, nullptr, 0)) { mfail(); return {}; }
        m_push_motion = true;      // simulate() re-installs its own table (or none), also after a failure below
        if (!marshal::annotate_chunks(m_ctx, poses.data(), n, m_n_objects, npx, extent_mask, out->notes, out->skipped, want_images ? &px : nullptr)) {
            fail(); return {};
        }
        for (size_t k = 0; want_images && k < n; k++) out->images.push_back(image(&px[k * npx], stamp));
        return out;
    }
    const std::string& lastError() const { return m_err; }
    // radar_tools/radar_img_to_pcl (launch/tests/radar_sim_test.launch:80-84, outside the checkout) on the GPU: one mono8
    // polar image of this model's shape (simulated or real) -> its detections, a PointCloud's points plus the intensity
    // channel (and the column / bin each came from), sorted by column, then bin.  The detector is this build's own
    // (rr_detect_config, include/radarays_mi355.h).  Empty on error (lastError()).
    std::vector<rr_radar_point> detect(const ImagePtr& image, const rr_detect_config& cfg)
    {
        std::vector<rr_radar_point> pts;
        if (!image || !push()) return pts;
        if (image->height != (uint32_t)m_cfg.n_cells || image->width != (uint32_t)m_n_angles || image->data.size() != (size_t)image->height * image->width) {
            m_err = "detect: the image is not n_cells x n_angles mono8"; std::cout << "[RadarHIP] " << m_err << std::endl; return pts;
        }
        std::vector<uint32_t> offs((size_t)m_n_angles + 1);
        if (rr_detect(m_ctx, image->data.data(), 1, &cfg, nullptr, 0, offs.data())) { fail(); return pts; }      // count
        pts.resize(offs.back());
        if (!pts.empty() && rr_detect(m_ctx, image->data.data(), 1, &cfg, pts.data(), (int)pts.size(), offs.data())) { fail(); pts.clear(); }
        return pts;
    }
    // ... by the windowed CFAR (rr_window_detect_config: a training window over range and azimuth under CA / GO / SO, or an ordered-statistic
    // threshold; rr_default_window_detect_config gives the defaults): the same points, and as asked for (non-null) the uint8 detection mask
    // [n_cells][n_angles], 255 at a detection, which labelComponents takes as it is.  ok (or null) tells an image without detections from an
    // error (lastError())
    std::vector<rr_radar_point> detectWindow(const ImagePtr& image, const rr_window_detect_config& cfg, std::vector<uint8_t>* mask = nullptr,
                                             bool* ok = nullptr)
    {
        std::vector<rr_radar_point> pts;
        if (ok) *ok = false;
        if (mask) mask->clear();
        if (!image || !push()) return pts;
        if (image->height != (uint32_t)m_cfg.n_cells || image->width != (uint32_t)m_n_angles || image->data.size() != (size_t)image->height * image->width) {
            m_err = "detectWindow: the image is not n_cells x n_angles mono8"; std::cout << "[RadarHIP] " << m_err << std::endl; return pts;
        }
        if (!marshal::detect_window(m_ctx, image->data.data(), image->data.size(), m_n_angles, cfg, pts, mask)) { fail(); return pts; }
        if (ok) *ok = true;
        return pts;
    }
    // the Cartesian bird's-eye image of one polar image: width x width mono8, forward = up, left = left, pixel_size m per pixel
    ImagePtr toCartesian(const ImagePtr& image, int width, float pixel_size, bool bilinear = true)
    {
        if (!image || !push()) return {};
        if (image->height != (uint32_t)m_cfg.n_cells || image->width != (uint32_t)m_n_angles || image->data.size() != (size_t)image->height * image->width) {
            m_err = "toCartesian: the image is not n_cells x n_angles mono8"; std::cout << "[RadarHIP] " << m_err << std::endl; return {};
        }
        rr_cartesian_config c{};
        c.width = width; c.interpolation = bilinear ? 1 : 0; c.pixel_size = pixel_size;
        ImagePtr msg = std::make_shared<Image>();
        msg->stamp = image->stamp; msg->frame_id = image->frame_id;
        msg->height = msg->width = msg->step = width > 0 ? (uint32_t)width : 0u;
        msg->data.resize((size_t)msg->height * msg->width);
        if (rr_polar_to_cartesian(m_ctx, image->data.data(), 1, &c, msg->data.data())) return fail();
        return msg;
    }
    // Sweep compensation (rr_deskew.hip; include/radarays_mi355.h): the record table of one sweep from its per-azimuth poses [n_angles][7]
    // (what simulateSweeps takes), the reference pose [7] and, with a non-zero Doppler gain, the sensor's map-frame velocity.  Empty on error
    std::vector<rr_sweep_rec> sweepTable(const std::vector<float>& az_poses, const float* ref_pose7, const float* sensor_vel3 = nullptr,
                                         float gain = 0.0f)
    {
        std::vector<rr_sweep_rec> table;
        if (!push()) return table;
        if (!ref_pose7 || az_poses.size() != 7 * (size_t)m_n_angles) { m_err = "sweepTable: the poses must be [n_angles][7]"; return table; }
        table.resize((size_t)m_n_angles);
        if (rr_sweep_table(m_ctx, az_poses.data(), ref_pose7, sensor_vel3, gain, 1, table.data())) { fail(); table.clear(); }
        return table;
    }
    // the detections of one image (detect(), with the offsets' total being their count) moved into the reference frame: same order, same
    // length; NaN for a point whose corrected range is not positive.  Empty on error
    std::vector<rr_radar_point> compensatePointClouds(const std::vector<rr_radar_point>& points, const std::vector<rr_sweep_rec>& table)
    {
        std::vector<rr_radar_point> out;
        if (points.empty() || !push()) return out;
        if (table.size() != (size_t)m_n_angles) { m_err = "compensatePointClouds: the table must be [n_angles]"; return out; }
        std::vector<uint32_t> offs((size_t)m_n_angles + 1, 0u);       // only the total is read
        offs.back() = (uint32_t)points.size();
        out.resize(points.size());
        if (rr_compensate_points(m_ctx, points.data(), offs.data(), 1, (int)points.size(), table.data(), out.data())) { fail(); out.clear(); }
        return out;
    }
    // the bird's-eye image of one polar image in the reference frame of its sweep (toCartesian with the distortion taken out)
    ImagePtr compensatedCartesian(const ImagePtr& image, const std::vector<rr_sweep_rec>& table, int width, float pixel_size, bool bilinear = true,
                                  int iterations = 2)
    {
        if (!image || !push()) return {};
        if (image->height != (uint32_t)m_cfg.n_cells || image->width != (uint32_t)m_n_angles || image->data.size() != (size_t)image->height * image->width ||
            table.size() != (size_t)m_n_angles) {
            m_err = "compensatedCartesian: the image is not n_cells x n_angles mono8 or the table not [n_angles]";
            std::cout << "[RadarHIP] " << m_err << std::endl; return {};
        }
        rr_cartesian_config c{};
        c.width = width; c.interpolation = bilinear ? 1 : 0; c.pixel_size = pixel_size;
        ImagePtr msg = std::make_shared<Image>();
        msg->stamp = image->stamp; msg->frame_id = image->frame_id;
        msg->height = msg->width = msg->step = width > 0 ? (uint32_t)width : 0u;
        msg->data.resize((size_t)msg->height * msg->width);
        if (rr_polar_to_cartesian_sweep(m_ctx, image->data.data(), 1, &c, table.data(), iterations, msg->data.data())) return fail();
        return msg;
    }
    // Scan matching (rr_icp.hip; include/radarays_mi355.h): point clouds (detect() or compensatePointClouds() of simulated images) registered
    // against ONE real cloud by planar point-to-point ICP with a fixed iteration count, from the states `init` ([n][4] = c s tx ty per
    // cloud) or from the identity.  One rr_icp_rec per cloud: the transform that maps the cloud into the real cloud's frame, sse,
    // n_matched, flags (rr_register_points, through marshal::register_clouds).  Empty on error
    std::vector<rr_icp_rec> registerPointClouds(const std::vector<std::vector<rr_radar_point>>& clouds, const std::vector<rr_radar_point>& real,
                                                float gate = 1.0f, int iterations = 10, const std::vector<double>& init = {})
    {
        std::vector<rr_icp_rec> recs;
        if (clouds.empty() || !push()) return recs;
        if (!marshal::register_clouds(m_ctx, clouds, m_n_angles, real, init, gate, iterations, recs)) {
            size_t mp = 0;
            for (const auto& c : clouds) mp = std::max(mp, c.size());
            if (mp > 65536 || real.size() > 65536 || (!init.empty() && init.size() != 4 * clouds.size()))
                m_err = "registerPointClouds: a cloud of more than 65536 points, or init is not [n][4]";
            else fail();
            recs.clear();
        }
        return recs;
    }
    // Oriented surface points (rr_surfels.hip; include/radarays_mi355.h): clouds (detect() of scans) reduced to sparse surface points, per
    // occupied cell of cfg's grid the mean of the 3 x 3 block of cells around it and the unit normal of the block's scatter, facing the
    // sensor.  surfels[f]: cloud f's first max_surfels records in ascending cell order; counts [n][2]: kept (the TRUE total), flags
    // (RR_SURFELS_*).  false on error
    bool surfacePoints(const std::vector<std::vector<rr_radar_point>>& clouds, const rr_surfel_config& cfg, std::vector<std::vector<rr_surfel>>& surfels,
                       std::vector<uint32_t>& counts, int max_surfels = 4096)
    {
        surfels.clear(); counts.clear();
        if (!push()) return false;
        if (!marshal::surface_points(m_ctx, clouds, m_n_angles, cfg, max_surfels, surfels, counts)) {
            size_t mp = 0;
            for (const auto& c : clouds) mp = std::max(mp, c.size());
            if (clouds.empty() || mp > 65536 || max_surfels < 0) m_err = "surfacePoints: no cloud, a cloud of more than 65536 points, or max_surfels < 0";
            else fail();
            return false;
        }
        return true;
    }
    // ... and registerPointClouds with a point-to-line residual: the clouds registered against ONE target of surface points (surfacePoints
    // of the real cloud) by planar ICP with a fixed iteration count, from `init` ([n][4] = c s tx ty per cloud) or from the identity.  One
    // rr_icp_rec per cloud (sse in (1/65536 m)^2); the pose convention is registerPointClouds', so correctedPose applies.  Empty on error
    std::vector<rr_icp_rec> registerSurfacePoints(const std::vector<std::vector<rr_radar_point>>& clouds, const std::vector<rr_surfel>& target,
                                                  float gate = 1.0f, int iterations = 10, const std::vector<double>& init = {})
    {
        std::vector<rr_icp_rec> recs;
        if (!push()) return recs;
        if (!marshal::register_surfels(m_ctx, clouds, m_n_angles, target, init, gate, iterations, recs)) {
            size_t mp = 0;
            for (const auto& c : clouds) mp = std::max(mp, c.size());
            if (clouds.empty() || mp > 65536 || target.size() > 65536 || (!init.empty() && init.size() != 4 * clouds.size()))
                m_err = "registerSurfacePoints: no cloud, more than 65536 points or surface points, or init is not [n][4]";
            else fail();
            recs.clear();
        }
        return recs;
    }
    // Pose-graph optimisation (rr_graph.hip; include/radarays_mi355.h): the back end behind the matchers.  states [N][4] = c s tx ty per node
    // (e.g. the integrated odometry) are optimised in place against the edges -- edge k says that node j sits at (c, s, tx, ty) in node i's
    // frame: a record of registerPointClouds / registerSurfacePoints / refinePoses with target i and source j, as it comes -- by
    // cfg.iterations Gauss-Newton steps of cfg.cg_iterations CG steps each; cfg.robust_k > 0 weighs false closures down.  One rr_graph_rec
    // per step and one for the result (chi2, edges used and flagged, dead blocks, the CG step a solve stopped at).  Empty on error, and
    // the states keep their values
    std::vector<rr_graph_rec> optimizePoseGraph(std::vector<double>& states, const std::vector<uint8_t>& fixed, const std::vector<rr_graph_edge>& edges,
                                                const rr_graph_config& cfg)
    {
        std::vector<rr_graph_rec> recs;
        if (!marshal::optimize_graph(m_ctx, states, fixed, edges, cfg, recs)) {
            if (fixed.empty() || states.size() != 4 * fixed.size() || cfg.iterations < 0 || cfg.iterations > 256)
                m_err = "optimizePoseGraph: no node, states that are not [N][4] for N = fixed.size(), or iterations outside 0..256";
            else fail();
            recs.clear();
        }
        return recs;
    }
    // the pose hypothesis X_h (qx qy qz qw tx ty tz) whose simulated cloud gave `rec` against the real cloud, corrected: T = X^-1 X_h, so
    // the result is X_h T^-1 -- X_h turned by -atan2(s, c) about its own z axis and moved by -R^T t in its own axes
    static std::array<float, 7> correctedPose(const float* pose7, const rr_icp_rec& rec)
    {
        const double c = rec.c, s = rec.s, v[3] = { -(c * rec.tx + s * rec.ty), -(-s * rec.tx + c * rec.ty), 0.0 };
        const double u[3] = { pose7[0], pose7[1], pose7[2] }, w = pose7[3];
        const double uv[3] = { u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0] };
        const double uuv[3] = { u[1] * uv[2] - u[2] * uv[1], u[2] * uv[0] - u[0] * uv[2], u[0] * uv[1] - u[1] * uv[0] };
        const double half = -0.5 * std::atan2(s, c), bz = std::sin(half), bw = std::cos(half);
        std::array<float, 7> out;
        out[0] = (float)(u[0] * bw + u[1] * bz); out[1] = (float)(u[1] * bw - u[0] * bz);
        out[2] = (float)(w * bz + u[2] * bw); out[3] = (float)(w * bw - u[2] * bz);
        for (int k = 0; k < 3; k++) out[4 + k] = (float)(pose7[4 + k] + v[k] + 2.0 * (w * uv[k] + uuv[k]));
        return out;
    }
    // Likelihood field (rr_field.hip; include/radarays_mi355.h): the map that keyframe clouds make (detect() of simulated images), each
    // under its state -- [n][4] = c s tx ty, or empty for the identity -- as the exact saturated squared distance field [height][width].
    // Pose convention: a state maps a cloud's sensor frame into the map frame, q = [c -s; s c] p + (tx, ty).  Empty on error
    std::vector<uint16_t> buildLikelihoodField(const std::vector<std::vector<rr_radar_point>>& clouds, const std::vector<double>& states,
                                               const rr_field_config& cfg)
    {
        std::vector<uint16_t> field;
        if (!push()) return field;
        if (!marshal::build_field(m_ctx, clouds, states, m_n_angles, cfg, field)) {
            if (clouds.empty() || (!states.empty() && states.size() != 4 * clouds.size())) m_err = "buildLikelihoodField: no cloud, or states is not [n][4]";
            else fail();
            field.clear();
        }
        return field;
    }
    // Map refinement (rr_refine.hip; include/radarays_mi355.h): the nearest-cell table [height][width] of an occupancy map -- a grid of
    // rr_rasterize_points at threshold 1, a map of buildOccupancyMap at 129 --: per cell the linear index jy * width + jx of the nearest
    // occupied cell, 0xFFFFFFFF where none lies within cfg.max_dist.  Empty on error
    std::vector<uint32_t> buildNearestField(const std::vector<uint8_t>& occ, const rr_field_config& cfg, int threshold = 1)
    {
        std::vector<uint32_t> nearest;
        if (!push()) return nearest;
        if (!marshal::build_nearest(m_ctx, occ, threshold, cfg, nearest)) {
            if (cfg.width < 1 || cfg.height < 1 || occ.size() != (size_t)cfg.width * (size_t)cfg.height) m_err = "buildNearestField: the map must be [height][width]";
            else fail();
            nearest.clear();
        }
        return nearest;
    }
    // ... and ONE scan refined against that table from n_hyp starting states, every buffer in HBM and the caller's: d_init [n_hyp][4] f64 =
    // c s tx ty (a state maps the scan's sensor frame into the map frame), d_recs [n_hyp].  One launch on `stream` runs every iteration;
    // the call returns once it is enqueued, and a record's first 32 bytes are a state that rr_rasterize_points and rr_occupancy_update take
    // as they are.  false on error
    bool refinePoses(const rr_radar_point* d_scan, const uint32_t* d_count, int max_points, const double* d_init, int n_hyp, const uint32_t* d_nearest,
                     const rr_field_config& cfg, rr_icp_rec* d_recs, int iterations = 10, void* stream = nullptr)
    {
        if (!push()) return false;
        if (!marshal::refine_poses(m_ctx, d_scan, d_count, max_points, d_init, n_hyp, d_nearest, cfg, iterations, d_recs, stream)) {
            fail();
            return false;
        }
        return true;
    }
    // The beam model (rr_cast.hip; include/radarays_mi355.h), every buffer in HBM and the caller's: the map's field cast at n_hyp states --
    // d_states [n_hyp][4] f32 = c s tx ty (a state maps the sensor frame into the map frame), d_dirs [n_angles][2] f32 = cos sin per azimuth
    // index -- into d_ranges uint16 [n_hyp][n_angles], the expected bin of every azimuth (beam.bin_end: the ray meets nothing).  One launch on
    // `stream`; the call returns once it is enqueued.  false on error
    bool castMap(const float* d_states, int n_hyp, const float* d_dirs, const uint16_t* d_field, const rr_field_config& cfg, const rr_beam_config& beam,
                 uint16_t* d_ranges, void* stream = nullptr)
    {
        if (!push()) return false;
        if (!marshal::cast_map(m_ctx, d_states, n_hyp, d_dirs, d_field, cfg, beam, d_ranges, stream)) {
            fail();
            return false;
        }
        return true;
    }
    // ... and ONE scan's profile d_first_bin uint16 [n_angles] (rr_scan_profile_device) scored against those rays: one rr_beam_rec per state
    // into d_recs [n_hyp]; more n_agree is better, n_through counts the rays that saw through a wall of the map.  false on error
    bool scoreBeams(const uint16_t* d_first_bin, const float* d_states, int n_hyp, const float* d_dirs, const uint16_t* d_field,
                    const rr_field_config& cfg, const rr_beam_config& beam, rr_beam_rec* d_recs, void* stream = nullptr)
    {
        if (!push()) return false;
        if (!marshal::score_beams(m_ctx, d_first_bin, d_states, n_hyp, d_dirs, d_field, cfg, beam, d_recs, stream)) {
            fail();
            return false;
        }
        return true;
    }
    // Mesh maps (rr_slice.hip; include/radarays_mi355.h): the loaded mesh itself as the grid map [height][width] -- a 1 in every cell that some
    // triangle, under its object's current pose, touches inside the height band [z_lo, z_hi] (metres, map frame), on the first device's
    // context.  skip_objects: object ids left out entirely (the parked and moving objects of a dynamic scene); objects (or null): receives
    // the smallest object id per cell, 0xFFFFFFFF where nothing marks it; occ: a map [height][width] to accumulate into, or empty.  The map
    // goes on to rr_distance_field (scorePoses, castMap, scoreBeams) or buildNearestField (refinePoses) as it is.  Empty on error
    std::vector<uint8_t> buildMeshMap(const rr_field_config& cfg, float z_lo, float z_hi, const std::vector<uint32_t>& skip_objects = {},
                                      std::vector<uint32_t>* objects = nullptr, const std::vector<uint8_t>& occ = {})
    {
        const size_t cells = cfg.width > 0 && cfg.height > 0 ? (size_t)cfg.width * (size_t)cfg.height : 0;
        if (!occ.empty() && occ.size() != cells) { m_err = "buildMeshMap: the map to accumulate into must be [height][width]"; return {}; }
        std::vector<uint8_t> skip(skip_objects.empty() ? 0 : m_n_objects, 0);
        for (uint32_t o : skip_objects) {
            if (o >= m_n_objects) { m_err = "buildMeshMap: skip_objects names an object the mesh does not have"; return {}; }
            skip[o] = 1;
        }
        std::vector<uint8_t> map = occ.empty() ? std::vector<uint8_t>(cells, 0) : occ;
        if (objects) objects->assign(cells, 0xFFFFFFFFu);
        const rr_slice_config band = { z_lo, z_hi, 0, 0 };
        if (rr_slice_mesh(m_ctx, &band, &cfg, skip.empty() ? nullptr : skip.data(), map.data(), objects ? objects->data() : nullptr)) {
            fail();
            if (objects) objects->clear();
            return {};
        }
        return map;
    }
    // Connected components (rr_components.hip; include/radarays_mi355.h).  The returns of n polar images [n][n_cells][n_angles] mono8 grouped
    // into clusters: the components of the pixels >= threshold on the cylinder (the azimuth axis wraps; RR_COMP_SEAM marks a cluster across
    // the first and last column), clusters below min_pixels dropped.  clusters[a]: image a's first max_components records in ascending root
    // order; counts [n][2]: kept, dropped; labels (or null): [n][n_cells][n_angles], the smallest linear index of the pixel's cluster,
    // 0xFFFFFFFF elsewhere.  false on error
    bool clusterImages(const std::vector<uint8_t>& images, int n_images, int threshold, std::vector<std::vector<rr_component>>& clusters,
                       std::vector<uint32_t>& counts, std::vector<uint32_t>* labels = nullptr, int connectivity = 8, int min_pixels = 1,
                       int max_components = 4096)
    {
        const rr_components_config cfg = { m_cfg.n_cells, m_n_angles, threshold, connectivity, 1, min_pixels, max_components, 0 };
        if (!marshal::label_components(m_ctx, images, n_images, cfg, clusters, counts, labels, nullptr)) {
            if (n_images < 1 || images.size() != (size_t)n_images * (size_t)m_cfg.n_cells * (size_t)m_n_angles) m_err = "clusterImages: the images must be [n][n_cells][n_angles] mono8";
            else fail();
            return false;
        }
        return true;
    }
    // ... and the occupied cells (>= threshold) of a grid map [height][width] grouped into segments without wrap, segments below min_cells
    // dropped: the cleaned map (the input's bytes under every kept cell, 0 elsewhere) for rr_distance_field / buildNearestField / castMap at
    // the same threshold, and every kept segment's record in ascending root order.  Empty on error
    std::vector<uint8_t> segmentMap(const std::vector<uint8_t>& occ, const rr_field_config& grid, int threshold, std::vector<rr_component>& segments,
                                    int min_cells = 1, int connectivity = 8)
    {
        std::vector<std::vector<rr_component>> comps;
        std::vector<uint32_t> counts;
        std::vector<uint8_t> clean;
        rr_components_config cfg = { grid.height, grid.width, threshold, connectivity, 0, min_cells, 4096, 0 };
        segments.clear();
        for (int round = 0; round < 2; round++) {                  // (a second time, with room for every record, when there are more than 4096)
            if (!marshal::label_components(m_ctx, occ, 1, cfg, comps, counts, nullptr, &clean)) {
                if (grid.width < 1 || grid.height < 1 || occ.size() != (size_t)grid.width * (size_t)grid.height) m_err = "segmentMap: the map must be [height][width]";
                else fail();
                return {};
            }
            if (counts[0] <= (uint32_t)cfg.max_components) break;
            cfg.max_components = (int32_t)counts[0];
        }
        segments = comps[0];
        return clean;
    }
    // one observed scan against hypothesis states [n][4] f32 (each the scan's sensor frame into the map frame) and a field of
    // buildLikelihoodField: one rr_field_rec per hypothesis, lower sum_d2 is better.  Empty on error
    std::vector<rr_field_rec> scorePoses(const std::vector<rr_radar_point>& scan, const std::vector<float>& states, const std::vector<uint16_t>& field,
                                         const rr_field_config& cfg)
    {
        std::vector<rr_field_rec> recs;
        if (!push()) return recs;
        if (!marshal::score_poses(m_ctx, scan, states, field, cfg, recs)) {
            if (states.empty() || states.size() % 4 || cfg.width < 1 || cfg.height < 1 || field.size() != (size_t)cfg.width * (size_t)cfg.height)
                m_err = "scorePoses: states must be [n][4] and the field [height][width]";
            else fail();
            recs.clear();
        }
        return recs;
    }
    // Correlative scan matching (rr_correlate.hip; include/radarays_mi355.h): one observed scan searched over a WIDE window around a coarse
    // candidate -- every yaw of `yaws` (radians) and every whole-cell offset |dx| <= corr.half_x, |dy| <= corr.half_y of the scan anchored
    // at (centre_x, centre_y) -- against a field of buildLikelihoodField.  The record holds the winner (rot indexes yaws; dx, dy in cells),
    // its score as scorePoses counts it, and what the search cost per level; pose_xyyaw (or null) receives the winner's metric pose
    // (centre_x + dx * cell, centre_y + dy * cell, yaws[rot]): the start for refinePoses.  The pruning is exact: corr.levels = 0 searches
    // every node and gives the same record apart from the counts.  Pose convention: an anchor state maps the scan's sensor frame into the
    // map frame.  false on error
    bool correlateScan(const std::vector<rr_radar_point>& scan, const std::vector<double>& yaws, double centre_x, double centre_y,
                       const std::vector<uint16_t>& field, const rr_field_config& cfg, const rr_corr_config& corr, rr_corr_rec& rec,
                       double* pose_xyyaw = nullptr)
    {
        rec = rr_corr_rec{};
        std::vector<float> rot;                                    // (the call needs neither the config nor the scene: nothing is pushed)
        for (double yaw : yaws) {
            rot.push_back((float)std::cos(yaw)); rot.push_back((float)std::sin(yaw));
            rot.push_back((float)centre_x); rot.push_back((float)centre_y);
        }
        if (!marshal::correlate_scan(m_ctx, scan, rot, field, cfg, corr, rec)) {
            if (yaws.empty() || cfg.width < 1 || cfg.height < 1 || field.size() != (size_t)cfg.width * (size_t)cfg.height)
                m_err = "correlateScan: yaws must not be empty and the field must be [height][width]";
            else fail();
            return false;
        }
        if (pose_xyyaw) {
            pose_xyyaw[0] = centre_x + (double)rec.dx * (double)cfg.cell;
            pose_xyyaw[1] = centre_y + (double)rec.dy * (double)cfg.cell;
            pose_xyyaw[2] = yaws[(size_t)rec.rot];
        }
        return true;
    }
    // Occupancy mapping (rr_occupancy.hip; include/radarays_mi355.h): n clouds (detect() of scans: sorted by column, then bin), each under
    // its state -- [n][4] = c s tx ty, or empty for the identity -- fused into `evidence`, int32 [height][width]: a detection adds
    // occ_cfg.l_hit to its cell, every cell a scan saw to be empty loses occ_cfg.l_free.  An evidence vector of the grid's size is
    // accumulated into, any other is replaced by zeros first.  Returns the byte map clamp(128 + evidence, 0, 255) -- 128 unknown, below it
    // free, above it occupied -- which rr_distance_field takes at threshold 129.  Pose convention: a state maps a cloud's sensor frame
    // into the map frame, q = [c -s; s c] p + (tx, ty).  Empty on error
    std::vector<uint8_t> buildOccupancyMap(const std::vector<std::vector<rr_radar_point>>& clouds, const std::vector<double>& states,
                                           const rr_field_config& cfg, const rr_occupancy_config& occ_cfg, std::vector<int32_t>& evidence)
    {
        std::vector<uint8_t> map;
        if (!push()) return map;
        if (!marshal::build_occupancy(m_ctx, clouds, states, m_n_angles, cfg, occ_cfg, evidence, map)) {
            if (clouds.empty() || (!states.empty() && states.size() != 4 * clouds.size())) m_err = "buildOccupancyMap: no cloud, or states is not [n][4]";
            else if (!std::all_of(clouds.begin(), clouds.end(), [&](const auto& c) { return marshal::sorted_by_column(c, m_n_angles); }))
                m_err = "buildOccupancyMap: a cloud is not sorted by column, or names a column past n_angles";
            else fail();
            map.clear();
        }
        return map;
    }
    // Particle filter step (rr_filter.hip; include/radarays_mi355.h): ONE scan and ONE particle set, both in HBM and the caller's, as every
    // buffer here is (d_recs [n], d_cum [n], d_ancestors [n], d_states_out [n][4], d_summary).  rr_score_poses_device,
    // rr_filter_resample_device and rr_filter_move_device run on `stream`; only the 32-byte summary comes back, in `summary`.  The
    // increment is the odometry (Dc, Ds, dx, dy) in the sensor frame.  n_eff_floor is the caller's resampling rule, decided here on the
    // host from `previous`, the summary of the step before (nullptr: resample): if its effective sample size total_weight^2 / sum_w2 is at
    // least n_eff_floor, every particle is kept and only moved.  The device never branches on it.  false on error
    bool filterStep(const rr_radar_point* d_scan, const uint32_t* d_count, int max_points, const float* d_states_in, int n, const uint16_t* d_field,
                    const rr_field_config& cfg, const uint16_t* d_table, const rr_filter_config& filter_cfg, const float (&increment)[4],
                    rr_field_rec* d_recs, uint64_t* d_cum, uint32_t* d_ancestors, float* d_states_out, rr_filter_summary* d_summary,
                    rr_filter_summary& summary, double n_eff_floor = 0.0, const rr_filter_summary* previous = nullptr, void* stream = nullptr)
    {
        if (!push()) return false;
        bool resample = true;
        if (previous && n_eff_floor > 0.0 && previous->sum_w2 > 0)
            resample = (double)previous->total_weight * (double)previous->total_weight / (double)previous->sum_w2 < n_eff_floor;
        if (!marshal::filter_step(m_ctx, d_scan, d_count, max_points, d_states_in, n, d_field, cfg, d_table, filter_cfg, increment, resample, d_recs,
                                  d_cum, d_ancestors, d_states_out, d_summary, stream, summary)) {
            fail();
            return false;
        }
        return true;
    }
    const rr_stats& lastStats() const { return m_stats; }

private:
    std::vector<ImagePtr> batch(const std::vector<float>& poses, bool sweeps, double stamp)
    {
        std::vector<ImagePtr> out;
        if (!push()) return out;
        const size_t per = sweeps ? 7 * (size_t)m_n_angles : 7;
        if (poses.empty() || poses.size() % per) { m_err = "poses must be [n][7] (sweeps: [n][n_angles][7])"; return out; }
        // on an error: the frames of the chunks before it are kept, and the text is reported whichever call failed
        if (!marshal::render_chunks(m_multi, poses.data(), poses.size() / per, sweeps, m_n_angles, (size_t)m_cfg.n_cells * m_n_angles,
                                    [&](const uint8_t* px, size_t) { out.push_back(image(px, stamp)); })) mfail();
        m_push_motion = true;      // simulate() re-installs its own table (or none)
        return out;
    }
    // n_cells x n_angles mono8 as RadarCPU.cpp:555-561 fills it; px null: zeros, to be rendered into
    ImagePtr image(const uint8_t* px, double stamp) const
    {
        ImagePtr msg = std::make_shared<Image>();
        msg->height = (uint32_t)m_cfg.n_cells; msg->width = (uint32_t)m_n_angles; msg->step = msg->width;
        const size_t npx = (size_t)msg->height * msg->width;
        if (px) msg->data.assign(px, px + npx); else msg->data.assign(npx, 0);
        msg->stamp = stamp; msg->frame_id = m_sensor_frame;
        return msg;
    }
    // marshal the protected state of Radar into the context (what simulate() reads, Radar.hpp:66-105)
    bool push()
    {
        if (m_resample || m_waves_start.empty()) {    // RadarCPU.cpp:136-145
            // the reference seeds every re-draw from std::random_device (radar_algorithms.cpp:258-259); so does this, unless
            // setBeamSeed fixed one -- and the seed that was USED is kept, so that a parameter batch can repeat the draw for
            // other beam widths on the same variates (advisor, round 4)
            if (!m_have_seed) m_beam_seed = (uint32_t)std::random_device{}();
            if (!marshal::draw_beam(m_beam_seed, m_params.model.beam_width, m_params.model.n_samples, m_cfg.beam_sample_dist,
                                    (float)m_cfg.beam_sample_dist_normal_p_in_cone, m_waves_start)) {
                m_err = "sample_cone_local: beam_sample_dist must be 0..3"; std::cout << "[RadarHIP] " << m_err << std::endl; return false;
            }
            m_resample = false; m_push_beams = true;
        }
        if (m_dirty_cfg) {
            rr_config c;       // n_angles / theta_min / theta_inc: the defaults
            marshal::fill_config(c, m_cfg, (int)m_params.model.n_reflections, m_wave_energy_threshold);
            if (rr_multi_set_config(m_multi, &c)) { mfail(); return false; }
            m_n_angles = c.n_angles; m_dirty_cfg = false; m_push_motion = true;
        }
        if (m_push_motion) {
            const bool on = m_cfg.include_motion && m_motion.size() == 7 * (size_t)m_n_angles;
            if (rr_multi_set_motion_poses(m_multi, on ? m_motion.data() : nullptr, on ? (size_t)m_n_angles : 0)) { mfail(); return false; }
            m_push_motion = false;
        }
        if (m_dirty_mat) {
            std::vector<rr_material> mats;
            marshal::append_materials(mats, m_params.materials.begin(), m_params.materials.end());
            const std::vector<int32_t> om = marshal::object_material_ids(m_object_materials);
            if (rr_multi_set_materials(m_multi, mats.data(), mats.size(), om.data(), om.size(), m_material_id_air)) { mfail(); return false; }
            m_dirty_mat = false;
        }
        if (m_push_beams) {
            if (rr_multi_set_beam_samples(m_multi, m_waves_start.data(), m_waves_start.size() / 3)) { mfail(); return false; }
            m_push_beams = false;
        }
        return true;
    }
    ImagePtr fail() { m_err = rr_last_error(m_ctx); std::cout << "[RadarHIP] " << m_err << std::endl; return {}; }
    void mfail() { m_err = rr_multi_last_error(m_multi); std::cout << "[RadarHIP] " << m_err << std::endl; }
    rr_multi* m_multi = nullptr;     // owns one context per device (and the RCCL communicator when there are several)
    rr_ctx* m_ctx = nullptr;         // = the context of the first device (statistics, parameter batches)
    std::vector<float> m_motion; bool m_push_motion = false;
    int m_n_angles = 400;
    size_t m_n_objects = 1;            // the mesh's: the largest face_object id + 1
    bool m_push_beams = false;
    uint32_t m_beam_seed = 0; bool m_have_seed = false;
    rr_stats m_stats{};
    std::string m_err;
};

}  // namespace radarays_ros_amd
