/*
 * ref_loop_wrap.cpp -- TEST INFRASTRUCTURE ONLY.
 *
 * Plain-C entry points around the reference's own C++ loop.  `make -C oracle ref` compiles this file together with the
 * reference's RadarCPU.cpp and radar_algorithms.cpp (read from the checkout at build time, never copied) against the
 * behaving stand-ins of oracle/refshim/ into oracle/_ref/libradarays_refloop.so.  What is defined here is the part of
 * the Radar base class that is not loop glue (its constructor, a pose lookup that steps through a caller's table) and a
 * subclass that reaches the protected state RadarCPU::simulate reads.  The nearest hit behind the stand-in simulator is
 * the oracle's orc_intersect, so a difference between this library and the oracle can only come from the loop.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <iostream>
#include <memory>
#include <random>
#include <sstream>
#include <vector>

#include "radarays_ros/RadarCPU.hpp"
#include <radarays_ros/image_algorithms.h>
#include <radarays_ros/radar_algorithms.h>

#include "radarays_oracle.h"

namespace rm = rmagine;
namespace rr = radarays_ros;

/* ---- the pose source that stands in for TF: a table the harness steps through ---- */
namespace {
const float* g_poses = nullptr;   /* [n][7] quaternion x, y, z, w + translation */
size_t g_n_poses = 0, g_pose_cursor = 0;
}

/* ROS names RadarCPU.cpp calls that tests/cpp/ros_stubs only declares */
void ros::spinOnce() {}

namespace radarays_ros {

/* The base class' constructor: the start values of Radar's state (400 azimuths, clockwise), without a parameter server
 * or a reconfigure server.  load() below overwrites all of it from the caller's tables. */
Radar::Radar(std::shared_ptr<ros::NodeHandle> nh_p, std::shared_ptr<tf2_ros::Buffer> tf_buffer,
             std::shared_ptr<tf2_ros::TransformListener> tf_listener, std::string map_frame, std::string sensor_frame)
    : m_nh_p(nh_p), m_tf_buffer(tf_buffer), m_tf_listener(tf_listener), has_last(false),
      m_map_frame(map_frame), m_sensor_frame(sensor_frame)
{
    m_cfg = RadarModelConfig();
    m_params.model.beam_width = 0.0f;
    m_params.model.n_samples = 0;
    m_params.model.n_reflections = 0;
    m_radar_model.phi = {0.0f, 1.0f, 1u};
    m_radar_model.theta = {0.0f, (float)(-(2.0 * M_PI) / 400.0), 400u};
    m_radar_model.range = {0.0f, 0.0f};
    m_polar_image = cv::Mat_<unsigned char>(0, 400);
}

/* One pose per call, in call order; the last one repeats.  Without motion the loop asks once per frame, with motion
 * once per azimuth. */
bool Radar::updateTsm()
{
    if (!g_poses || g_n_poses == 0) return false;
    const float* p = g_poses + 7 * (g_pose_cursor < g_n_poses ? g_pose_cursor : g_n_poses - 1);
    g_pose_cursor++;
    rm::Transform T;
    T.R.x = p[0]; T.R.y = p[1]; T.R.z = p[2]; T.R.w = p[3];
    T.t.x = p[4]; T.t.y = p[5]; T.t.z = p[6];
    Tsm_last = T;
    has_last = true;
    return true;
}

}  // namespace radarays_ros

namespace {

class Probe : public rr::RadarCPU {
public:
    explicit Probe(rm::EmbreeMapPtr map) : rr::RadarCPU(nullptr, nullptr, nullptr, "map", "sensor", map) {}

    void load(const orc_material* materials, size_t n_materials, const int32_t* object_materials, size_t n_objects,
              const orc_config* c, int include_motion, const float* beam_dirs, size_t n_beam)
    {
        m_cfg = rr::RadarModelConfig();
        m_cfg.n_cells = c->n_cells;
        m_cfg.n_reflections = c->n_reflections;
        m_cfg.n_samples = (int)n_beam;
        m_cfg.signal_denoising = c->signal_denoising;
        m_cfg.signal_denoising_triangular_width = c->signal_denoising_triangular_width;
        m_cfg.signal_denoising_gaussian_width = c->signal_denoising_gaussian_width;
        m_cfg.signal_denoising_mb_width = c->signal_denoising_mb_width;
        m_cfg.signal_denoising_triangular_mode = c->signal_denoising_triangular_mode;
        m_cfg.signal_denoising_gaussian_mode = c->signal_denoising_gaussian_mode;
        m_cfg.signal_denoising_mb_mode = c->signal_denoising_mb_mode;
        m_cfg.ambient_noise = c->ambient_noise;
        m_cfg.ambient_noise_at_signal_0 = c->ambient_noise_at_signal_0;
        m_cfg.ambient_noise_at_signal_1 = c->ambient_noise_at_signal_1;
        m_cfg.ambient_noise_energy_max = c->ambient_noise_energy_max;
        m_cfg.ambient_noise_energy_min = c->ambient_noise_energy_min;
        m_cfg.ambient_noise_energy_loss = c->ambient_noise_energy_loss;
        m_cfg.scroll_image = c->scroll_image;
        m_cfg.record_multi_reflection = c->record_multi_reflection != 0;
        m_cfg.record_multi_path = c->record_multi_path != 0;
        m_cfg.multipath_threshold = c->multipath_threshold;
        m_cfg.include_motion = include_motion != 0;
        m_cfg.resolution = c->resolution;
        m_cfg.energy_max = c->energy_max;
        m_cfg.signal_max = c->signal_max;

        m_params.materials.data.clear();
        for (size_t i = 0; i < n_materials; i++) {
            rr::RadarMaterial m;
            m.velocity = materials[i].velocity; m.ambient = materials[i].ambient;
            m.diffuse = materials[i].diffuse; m.specular = materials[i].specular;
            m_params.materials.data.push_back(m);
        }
        m_params.model.n_samples = (uint32_t)n_beam;
        m_params.model.n_reflections = (uint32_t)c->n_reflections;
        m_object_materials.assign(object_materials, object_materials + n_objects);
        m_material_id_air = c->material_id_air;
        m_wave_energy_threshold = c->wave_energy_threshold;

        m_radar_model.theta.min = c->theta_min;
        m_radar_model.theta.inc = c->theta_inc;
        m_radar_model.theta.size = (uint32_t)c->n_angles;
        m_polar_image = cv::Mat_<unsigned char>(0, c->n_angles);

        /* the beam samples are an input: no resampling */
        m_waves_start.clear();
        for (size_t i = 0; i < n_beam; i++) {
            rr::DirectedWave w;
            w.energy = 1.0; w.polarization = 0.5; w.frequency = 76.5; w.velocity = 0.3; w.material_id = 0; w.time = 0.0;
            w.ray.orig = rm::Vector::Zeros();
            w.ray.dir = {beam_dirs[3 * i], beam_dirs[3 * i + 1], beam_dirs[3 * i + 2]};
            m_waves_start.push_back(w);
        }
        m_resample = false;
    }
};

/* keeps the loop's progress lines off the caller's stdout */
struct QuietCout {
    std::ostringstream sink;
    std::streambuf* old;
    QuietCout() : old(std::cout.rdbuf(sink.rdbuf())) {}
    ~QuietCout() { std::cout.rdbuf(old); }
};

rr::DirectedWave wave_of(const float dir[3], double energy, double polarization, double velocity)
{
    rr::DirectedWave w;
    w.ray.orig = rm::Vector::Zeros();
    w.ray.dir = {dir[0], dir[1], dir[2]};
    w.energy = energy; w.polarization = polarization; w.velocity = velocity;
    w.frequency = 76.5; w.time = 0.0; w.material_id = 0;
    return w;
}

void copy_weights(const std::vector<float>& w, float* out)
{
    if (!w.empty()) memcpy(out, w.data(), w.size() * sizeof(float));
}

/* the first uniform f32 draw of a generator seeded with `seed`, times 1000 in f64: the noise offset the loop derives
 * from the seed its random device hands it */
double first_offset_of(uint32_t seed)
{
    std::mt19937 engine(seed);
    std::uniform_real_distribution<float> unit(0.0f, 1.0f);
    const float u = unit(engine);
    return (double)u * 1000.0;
}

}  // namespace

extern "C" {

/* One call of the reference's RadarCPU::simulate.  poses: [n_poses][7]; one pose without motion, one per azimuth with.
 * noise_seeds: what the loop's random device returns, in call order (one per azimuth when ambient_noise != 0); the seeds
 * actually handed out come back in seed_log.  out_u8: [n_cells][n_angles]. */
int ref_simulate(const orc_scene* scene, const uint32_t* face_object_id,
                 const orc_material* materials, size_t n_materials,
                 const int32_t* object_materials, size_t n_objects,
                 const orc_config* cfg, int include_motion,
                 const float* beam_dirs, size_t n_beam,
                 const float* poses, size_t n_poses,
                 const uint32_t* noise_seeds, size_t n_noise_seeds,
                 uint8_t* out_u8,
                 uint32_t* seed_log, size_t seed_log_cap, size_t* n_seed_log)
{
    if (!scene || !cfg || !poses || !n_poses || !out_u8) return -1;
    if (cfg->brdf_model != 0) return -3;   /* the build's own lobe has no counterpart in the reference */
    auto map = std::make_shared<rm::EmbreeMap>();
    map->scene = scene;
    map->face_object_id = face_object_id;
    Probe radar(map);
    radar.load(materials, n_materials, object_materials, n_objects, cfg, include_motion, beam_dirs, n_beam);

    g_poses = poses; g_n_poses = n_poses; g_pose_cursor = 0;
    refshim::seed_state& s = refshim::seeds();
    s.queue.assign(noise_seeds, noise_seeds + (noise_seeds ? n_noise_seeds : 0));
    s.log.clear();

    sensor_msgs::ImagePtr msg;
    {
        QuietCout quiet;
        msg = radar.simulate(ros::Time(0));
    }
    g_poses = nullptr; g_n_poses = 0;
    s.queue.clear();
    if (n_seed_log) *n_seed_log = s.log.size();
    for (size_t i = 0; seed_log && i < s.log.size() && i < seed_log_cap; i++) seed_log[i] = s.log[i];
    if (!msg) return -2;
    if (msg->height != (uint32_t)cfg->n_cells || msg->width != (uint32_t)cfg->n_angles) return -4;
    memcpy(out_u8, msg->data.data(), msg->data.size());
    return 0;
}

void ref_fresnel(const float normal[3], const float dir[3], double energy, double polarization, double v1, double v2,
                 float refl_dir[3], double* refl_energy, float refr_dir[3], double* refr_energy)
{
    const rm::Vector n = {normal[0], normal[1], normal[2]};
    const auto res = rr::fresnel(n, wave_of(dir, energy, polarization, v1), v2);
    refl_dir[0] = res.first.ray.dir.x; refl_dir[1] = res.first.ray.dir.y; refl_dir[2] = res.first.ray.dir.z;
    refr_dir[0] = res.second.ray.dir.x; refr_dir[1] = res.second.ray.dir.y; refr_dir[2] = res.second.ray.dir.z;
    *refl_energy = res.first.energy;
    *refr_energy = res.second.energy;
}

float ref_back_reflection_shader(float incidence_angle, float energy, float diffuse, float specular_fac, float specular_exp)
{
    return rr::back_reflection_shader(incidence_angle, energy, diffuse, specular_fac, specular_exp);
}

double ref_incidence_angle(const float normal[3], const float dir[3])
{
    const rm::Vector n = {normal[0], normal[1], normal[2]};
    return rr::get_incidence_angle(n, wave_of(dir, 1.0, 0.5, 0.3));
}

double ref_angle_between(const float a[3], const float b[3])
{
    const rm::Vector va = {a[0], a[1], a[2]}, vb = {b[0], b[1], b[2]};
    return rr::angle_between(va, vb);
}

void ref_make_denoiser_triangular(int width, int mode, float* out) { copy_weights(rr::make_denoiser_triangular(width, mode), out); }
void ref_make_denoiser_gaussian(int width, int mode, float* out) { copy_weights(rr::make_denoiser_gaussian(width, mode), out); }
void ref_make_denoiser_maxwell_boltzmann(int width, int mode, float* out) { copy_weights(rr::make_denoiser_maxwell_boltzmann(width, mode), out); }

double ref_perlin_noise(double x, double y, double z) { return rr::perlin_noise(x, y, z); }

void ref_wave_move(float orig[3], const float dir[3], double* time, double velocity, double distance)
{
    rr::DirectedWave w = wave_of(dir, 1.0, 0.5, velocity);
    w.ray.orig = {orig[0], orig[1], orig[2]};
    w.time = *time;
    const rr::DirectedWave m = w.move(distance);
    orig[0] = m.ray.orig.x; orig[1] = m.ray.orig.y; orig[2] = m.ray.orig.z;
    *time = m.time;
}

/* The reference's sample_cone_local with its random device handing out `seed`.  out_u / out_r: the variates its generator
 * drew for each sample (the angle's uniform, then the radius' uniform or normal), replayed here from the same seed with
 * the same standard-library classes, so that the oracle's variate-fed twin can be given the same inputs.
 * sample_dist outside 0..3 leaves the radius uninitialised in the reference and is refused. */
int ref_sample_cone_local(uint32_t seed, float width, int n_samples, int sample_dist, float p_in_cone,
                          float* out_dirs, float* out_u, float* out_r)
{
    if (sample_dist < 0 || sample_dist > 3 || n_samples < 0) return -1;
    refshim::seed_state& s = refshim::seeds();
    s.queue.assign(1, seed);
    s.log.clear();
    const float ahead[3] = {1.0f, 0.0f, 0.0f};
    const rr::DirectedWave start = wave_of(ahead, 1.0, 0.5, 0.3);
    const std::vector<rr::DirectedWave> waves = rr::sample_cone_local(start, width, n_samples, sample_dist, p_in_cone);
    s.queue.clear();
    if (s.log.size() != 1 || s.log[0] != seed || (int)waves.size() != n_samples) return -2;
    std::mt19937 engine(seed);
    std::uniform_real_distribution<float> unit(0.0f, 1.0f);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    for (int i = 0; i < n_samples; i++) {
        out_dirs[3 * i] = waves[i].ray.dir.x; out_dirs[3 * i + 1] = waves[i].ray.dir.y; out_dirs[3 * i + 2] = waves[i].ray.dir.z;
        out_u[i] = unit(engine);
        out_r[i] = sample_dist < 2 ? unit(engine) : gauss(engine);
    }
    return 0;
}

double ref_noise_offset(uint32_t seed) { return first_offset_of(seed); }

/* The build injects its noise offsets as f32; the loop's own offset is an f64 product.  Finds, from
 * `start` upwards, n seeds whose offset is exactly an f32, so that the oracle can be handed the very same number. */
void ref_find_noise_seeds(uint32_t start, size_t n, uint32_t* out_seeds, float* out_offsets)
{
    uint32_t seed = start;
    for (size_t i = 0; i < n; seed++) {
        const double off = first_offset_of(seed);
        if ((double)(float)off == off) { out_seeds[i] = seed; out_offsets[i] = (float)off; i++; }
    }
}

/* The uniform variates the loop draws per cell for ambient_noise == 1 after its offset draw, replayed from the seed. */
void ref_uniform_stream(uint32_t seed, size_t n, float* out)
{
    std::mt19937 engine(seed);
    std::uniform_real_distribution<float> unit(0.0f, 1.0f);
    (void)unit(engine);
    for (size_t i = 0; i < n; i++) out[i] = unit(engine);
}

}  // extern "C"
