// rr_api.hip -- C ABI of libradarays_mi355.so (include/radarays_mi355.h): the context's life, its parameter tables and their upload, synchronisation and errors,
// page-locked memory; the rest is rr_scene.hip, rr_frame.hip, rr_side.hip, rr_sets.hip, rr_images.hip, rr_probe.hip.  No CPU fallback: a compute call runs the gfx950 kernels or fails with an error string.
#include "rr_ctx.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <dlfcn.h>

namespace rr {
namespace {

std::string g_create_error;

bool roctx_load()
{
    static int state = 0;   // 0 untried, 1 ok, -1 missing
    if (state == 0) {
        state = -1;
        for (const char* n : { "librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so" }) {
            void* h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            g_roctx_push = (roctx_push_fn)dlsym(h, "roctxRangePushA");
            g_roctx_pop = (roctx_pop_fn)dlsym(h, "roctxRangePop");
            if (g_roctx_push && g_roctx_pop) { state = 1; break; }
        }
    }
    return state == 1;
}

// radar_algorithms.h:283-351 + RadarCPU.cpp:48-93 (host, same float/double mix)
void make_smear(const rr_config& cfg, std::vector<float>& w, int& mode)
{
    w.clear(); mode = 0;
    int width = 0; double mfrac = 0.0;
    if (cfg.signal_denoising == 1) { width = cfg.signal_denoising_triangular_width; mfrac = cfg.signal_denoising_triangular_mode; }
    else if (cfg.signal_denoising == 2) { width = cfg.signal_denoising_gaussian_width; mfrac = cfg.signal_denoising_gaussian_mode; }
    else if (cfg.signal_denoising == 3) { width = cfg.signal_denoising_mb_width; mfrac = cfg.signal_denoising_mb_mode; }
    if (width <= 0) return;
    mode = (int)(mfrac * width);
    w.resize((size_t)width);
    if (cfg.signal_denoising == 3) {
        const float fm = (float)mode;
        const float a = (float)((double)fm / M_SQRT2);
        for (int i = 0; i < width; i++) {
            const float x = (float)i;
            const float xx = x * x, aa = a * a, aaa = a * a * a;
            w[i] = (float)(std::sqrt(2.0 / M_PI) * (double)xx * (double)expf(-xx / (2 * aa)) / (double)aaa);
        }
    } else {
        for (int i = 0; i < width; i++) {
            float p;
            if (i <= mode) p = (float)i / (float)mode;
            else p = (float)(1.0 - (double)(((float)i - (float)mode) / ((float)width - (float)mode)));
            w[i] = (float)((double)(p * 1.0f) + (1.0 - (double)p) * (double)0.0f);
        }
    }
    float sum = 0.0f;
    for (int i = 0; i < width; i++) sum += w[i];
    for (int i = 0; i < width; i++) w[i] /= sum;
    const double mode_val = w[mode];
    for (int i = 0; i < width; i++) w[i] = (float)((double)w[i] / mode_val);
}

// the context's page-locked block (upload_table, read_back) with room for `bytes`
hipError_t ensure_h_rb(rr_ctx* c, size_t bytes)
{
    if (c->h_rb_bytes >= bytes) return hipSuccess;
    if (c->h_rb) (void)hipHostFree(c->h_rb);
    c->h_rb = nullptr; c->h_rb_bytes = 0;
    hipError_t e = hipHostMalloc(&c->h_rb, bytes + 4096, hipHostMallocDefault);
    if (e == hipSuccess) c->h_rb_bytes = bytes + 4096;
    return e;
}

// a set-up table goes up through a page-locked staging block and a word-copy kernel on the NULL stream (ordered exactly like the
// hipMemcpy it replaces, and complete on return): no dispatch of the runtime's own copy kernel is left in a run's kernel trace.
// Larger than 4 MB, or not whole words: hipMemcpy
hipError_t upload_table(rr_ctx* c, void* d_dst, const void* src, size_t bytes)
{
    if (bytes == 0) return hipSuccess;
    if (bytes % 4 != 0 || bytes > ((size_t)4 << 20)) return hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice);
    hipError_t e = ensure_h_rb(c, bytes);
    if (e != hipSuccess) return e;
    std::memcpy(c->h_rb, src, bytes);
    launch_copy_words(c->h_rb, d_dst, bytes, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}

// the one angle of total reflection that does not depend on the material table (rr_create)
int limit_of_same_material(rr_ctx* c)
{
    const float4 same = make_float4(0.3f, 0.f, 0.f, 0.f);
    DevBuf<float4> m1; DevBuf<double> l1;
    RR_HIP(c, m1.ensure(1)); RR_HIP(c, l1.ensure(2));
    RR_HIP(c, upload_table(c, m1.p, &same, sizeof(same)));
    launch_mat_limits(m1.p, 1, l1.p, nullptr);
    RR_HIP(c, hipStreamSynchronize(nullptr));
    double two[2] = {0.0, 0.0};
    const int rc = read_back(c, two, l1.p, sizeof(two));
    c->limit_same = two[0];
    return rc;
}

}  // namespace

int fail(rr_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

// trace orders of a beam table (results are always stored under the reference index, so they only change speed):
//   pass 0     : k_trace tiles (beam sample, azimuth) into waves itself (see there); this order
//                decides which samples share a tile / are neighbours in the launch: rows of nearly
//                equal elevation, sorted by yaw inside a row
//   pass 1 ... : inherited through torder from a second order of the beam samples, yaw-major rows
//                (the reflected fan of a yaw slice stays together; measured against elevation-major
//                and Morton orders)
void beam_trace_orders(const float* beams, size_t nb, std::vector<uint32_t>& order, std::vector<uint32_t>& order2)
{
    auto make_order = [&](int major, std::vector<uint32_t>& o) {   // major: 2 = elevation (z), 1 = yaw (y)
        o.resize(nb);
        for (size_t i = 0; i < nb; i++) o[i] = (uint32_t)i;
        const int minor = 3 - major;
        std::stable_sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return beams[3 * a + major] < beams[3 * b + major]; });
        for (size_t i = 0; i < nb; i += 16)
            std::stable_sort(o.begin() + i, o.begin() + std::min(nb, i + 16), [&](uint32_t a, uint32_t b) { return beams[3 * a + minor] < beams[3 * b + minor]; });
    };
    make_order(2, order);
    make_order(1, order2);
}

int upload_tables(rr_ctx* c)
{
    if (!c->tables_dirty) return 0;
    RR_HIP(c, hipDeviceSynchronize());   // frames in flight on the lanes still read the old tables
    const rr_config& g = c->cfg;
    const unsigned dirty = c->tables_dirty;
    if (dirty & (rr_ctx::D_CFG | rr_ctx::D_BEAMS | rr_ctx::D_MAT)) c->hist_gen++;     // wave counts per pass change: the trace-grid history starts over
    // captured launches (launch graphs) hold table pointers and scalars of the old parameters.  Fresh noise offsets or motion
    // tables of the SAME shape -- what a node sets before every frame (RadarCPU.cpp:461-472, :190-196) -- only change the
    // contents of a buffer the graphs already point at
    bool regen = (dirty & (rr_ctx::D_CFG | rr_ctx::D_BEAMS | rr_ctx::D_MAT)) != 0;
    const void* noise_before = c->d_noise.p; const int noise_rows_before = c->noise_rows;
    const void* motion_before = c->motion_live ? (const void*)c->d_motion.p : nullptr; const int motion_rows_before = c->motion_rows;
    if (dirty & rr_ctx::D_CFG) {
    // Tas.R = EulerAngles{0,0,theta(angle)} -> quaternion (rmagine ZYX), RadarCPU.cpp:202
    std::vector<float4> qas((size_t)g.n_angles);
    for (int k = 0; k < g.n_angles; k++) {
        const float theta = g.theta_min + (float)k * g.theta_inc;
        const float roll = 0.0f, pitch = 0.0f, yaw = theta;
        const float cr = cosf(roll / 2.0f), sr = sinf(roll / 2.0f);
        const float cp = cosf(pitch / 2.0f), sp = sinf(pitch / 2.0f);
        const float cy = cosf(yaw / 2.0f), sy = sinf(yaw / 2.0f);
        float4 q;
        q.w = cr * cp * cy + sr * sp * sy;
        q.x = sr * cp * cy - cr * sp * sy;
        q.y = cr * sp * cy + sr * cp * sy;
        q.z = cr * cp * sy - sr * sp * cy;
        qas[k] = q;
    }
    RR_HIP(c, c->d_qas.ensure(qas.size()));
    RR_HIP(c, upload_table(c, c->d_qas.p, qas.data(), qas.size() * sizeof(float4)));
    }

    if (dirty & rr_ctx::D_BEAMS) {
    const size_t nb = c->beams.size() / 3;
    std::vector<float4> b4(nb);
    for (size_t i = 0; i < nb; i++) b4[i] = make_float4(c->beams[3 * i], c->beams[3 * i + 1], c->beams[3 * i + 2], 0.0f);
    RR_HIP(c, c->d_beams.ensure(nb));
    if (nb) RR_HIP(c, upload_table(c, c->d_beams.p, b4.data(), nb * sizeof(float4)));
    {
        std::vector<uint32_t> order, order2;
        beam_trace_orders(c->beams.data(), nb, order, order2);
        RR_HIP(c, c->d_beam_order2.ensure(nb));
        if (nb) RR_HIP(c, upload_table(c, c->d_beam_order2.p, order2.data(), nb * sizeof(uint32_t)));
        RR_HIP(c, c->d_beam_order.ensure(nb));
        if (nb) RR_HIP(c, upload_table(c, c->d_beam_order.p, order.data(), nb * sizeof(uint32_t)));
    }
    }

    if (dirty & rr_ctx::D_MAT) {
    std::vector<float4> m4(c->materials.size());
    for (size_t i = 0; i < m4.size(); i++)
        m4[i] = make_float4(c->materials[i].velocity, c->materials[i].ambient, c->materials[i].diffuse, c->materials[i].specular);
    RR_HIP(c, c->d_materials.ensure(m4.size()));
    if (!m4.empty()) RR_HIP(c, upload_table(c, c->d_materials.p, m4.data(), m4.size() * sizeof(float4)));
    // angles of total reflection, tabulated on the device (the very asin the kernels used to call per wave-pass)
    RR_HIP(c, c->d_mat_limits.ensure(m4.size()));
    launch_mat_limits(c->d_materials.p, m4.size(), c->d_mat_limits.p, nullptr);
    RR_HIP(c, hipGetLastError());
    // the frame streams are non-blocking: nothing orders them behind the NULL stream this table was launched on
    RR_HIP(c, hipStreamSynchronize(nullptr));
    RR_HIP(c, c->d_objmat.ensure(c->object_materials.size()));
    if (!c->object_materials.empty())
        RR_HIP(c, upload_table(c, c->d_objmat.p, c->object_materials.data(), c->object_materials.size() * sizeof(int32_t)));
    }

    if (dirty & rr_ctx::D_CFG) {
    make_smear(g, c->smear, c->smear_mode);
    RR_HIP(c, c->d_smear.ensure(c->smear.size()));
    if (!c->smear.empty()) RR_HIP(c, upload_table(c, c->d_smear.p, c->smear.data(), c->smear.size() * sizeof(float)));

    RR_HIP(c, c->d_decay.ensure((size_t)std::max(1, g.n_cells)));
    launch_decay_table(c->d_decay.p, g.n_cells, g.resolution, g.ambient_noise_energy_loss, nullptr);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipDeviceSynchronize());
    }

    if (dirty & (rr_ctx::D_NOISE | rr_ctx::D_CFG)) {
    // one row of n_angles offsets, or k rows: frame f of a batch then takes row f % k (the reference draws
    // fresh offsets for every frame, RadarCPU.cpp:461-472)
    const size_t A = (size_t)g.n_angles;
    if (!c->noise.empty() && c->noise.size() % A != 0)
        return fail(c, -3, "rr_set_noise_offsets: the number of offsets must be a multiple of n_angles (one row per frame of a batch)");
    c->noise_rows = c->noise.size() >= 2 * A ? (int)(c->noise.size() / A) : 1;
    std::vector<float> nz((size_t)c->noise_rows * A, 0.0f);
    for (size_t i = 0; i < nz.size() && i < c->noise.size(); i++) nz[i] = c->noise[i];
    RR_HIP(c, c->d_noise.ensure(nz.size()));
    RR_HIP(c, upload_table(c, c->d_noise.p, nz.data(), nz.size() * sizeof(float)));
    }
    if ((dirty & (rr_ctx::D_MOTION | rr_ctx::D_CFG)) && !c->motion.empty()) {
        // one table of n_angles poses, or k tables: frame f of a batch then takes table f % k (one sweep of the antenna per frame)
        if (c->motion.size() % (7 * (size_t)g.n_angles) != 0)
            return fail(c, -3, "rr_set_motion_poses: the number of poses must be a multiple of n_angles (one table per frame of a batch)");
        c->motion_rows = (int)(c->motion.size() / (7 * (size_t)g.n_angles));
        RR_HIP(c, c->d_motion.ensure(c->motion.size()));
        RR_HIP(c, upload_table(c, c->d_motion.p, c->motion.data(), c->motion.size() * sizeof(float)));
    }
    c->motion_live = !c->motion.empty();
    const void* motion_after = c->motion_live ? (const void*)c->d_motion.p : nullptr;
    if (regen || noise_before != (const void*)c->d_noise.p || noise_rows_before != c->noise_rows ||
        motion_before != motion_after || motion_rows_before != c->motion_rows) c->graph_gen++;
    c->tables_dirty = 0;
    return 0;
}

// a small synchronous read-back of device words (counters, per-pass statistics) without asking the runtime for a copy: a kernel
// stores them into a page-locked block of the context, the host copies from there.  The device must be idle on these words
// (the callers have synchronised).  Sizes that are not multiples of 16 take hipMemcpy
int read_back(rr_ctx* c, void* dst, const void* d_src, size_t bytes)
{
    if (bytes == 0) return 0;
    if (bytes % 16 != 0 || (uintptr_t)d_src % 16 != 0) { RR_HIP(c, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost)); return 0; }
    RR_HIP(c, ensure_h_rb(c, bytes));
    launch_copy_host(d_src, c->h_rb, bytes, 4, -1, c->stream);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipStreamSynchronize(c->stream));
    std::memcpy(dst, c->h_rb, bytes);
    return 0;
}

// a frame's error bits (Counters::overflow, the lanes' sticky words) as the failure of the call that reports them
int overflow_error(rr_ctx* c, uint32_t bits, bool since_sync)
{
    if (bits & 1u)
        return fail(c, -7, std::string("wave/signal queue capacity exceeded") + (since_sync ? " in a frame since the last rr_synchronize" : "") +
                               "; raise rr_config.max_waves_per_azimuth");
    if (bits & 2u)
        return fail(c, -8, std::string("object id or material id out of range of the tables given to rr_set_materials") +
                               (since_sync ? " (a frame since the last rr_synchronize)" : ""));
    return 0;
}

int check_ready(rr_ctx* c)
{
    if (!c) return -1;
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    if (!c->have_cfg) return fail(c, -2, "rr_set_config has not been called");
    if (!c->have_materials) return fail(c, -2, "rr_set_materials has not been called");
    if (c->beams.empty() && c->cfg.n_reflections > 0) return fail(c, -2, "rr_set_beam_samples has not been called");
    return 0;
}

}  // namespace rr

// ---------------------------------------------------------------------------
extern "C" {

int rr_abi_version(void) { return RR_ABI_VERSION; }

void rr_partition(int n_angles, int world, int rank, int* begin, int* end)
{
    // contiguous azimuth blocks that differ by at most one column (radarays_ros_amd/dist.py: partition)
    if (world < 1) world = 1;
    const int base = n_angles / world, rem = n_angles % world;
    const int b = rank * base + (rank < rem ? rank : rem);
    if (begin) *begin = b;
    if (end) *end = b + base + (rank < rem ? 1 : 0);
}

void rr_default_config(rr_config* cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->n_cells = 3424; cfg->n_angles = 400; cfg->n_reflections = 4;
    cfg->signal_denoising = 1;
    cfg->signal_denoising_triangular_width = 50; cfg->signal_denoising_triangular_mode = 0.35;
    cfg->signal_denoising_gaussian_width = 50; cfg->signal_denoising_gaussian_mode = 0.5;
    cfg->signal_denoising_mb_width = 50; cfg->signal_denoising_mb_mode = 0.4;
    cfg->ambient_noise = 2; cfg->scroll_image = 0;
    cfg->record_multi_reflection = 1; cfg->record_multi_path = 0;
    cfg->max_waves_per_azimuth = 0;
    cfg->resolution = 0.0438; cfg->energy_max = 0.5; cfg->signal_max = 120.0;
    cfg->ambient_noise_at_signal_0 = 0.3; cfg->ambient_noise_at_signal_1 = 0.03;
    cfg->ambient_noise_energy_max = 0.5; cfg->ambient_noise_energy_min = 0.1;
    cfg->ambient_noise_energy_loss = 0.05; cfg->multipath_threshold = 0.5;
    cfg->wave_energy_threshold = 0.001f;
    cfg->theta_min = 0.0f; cfg->theta_inc = (float)(-(2 * M_PI) / 400);
    cfg->range_max = 1000.0f;
}

rr_ctx* rr_create(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_error = std::string("rr_create: no HIP device (") + (e != hipSuccess ? hipGetErrorString(e) : "count 0") +
                         "); this library has no CPU fallback";
        return nullptr;
    }
    if (device < 0 || device >= n) { g_create_error = "rr_create: device index out of range"; return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "rr_create: hipSetDevice failed"; return nullptr; }
    rr_ctx* c = new rr_ctx();
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        g_create_error = "rr_create: hipStreamCreate failed"; delete c; return nullptr;
    }
    rr_default_config(&c->cfg);
    // 4 buffer sets: the sharded step loop (dist.py) keeps 4 steps in flight on its own streams
    // (measured optimum: 4 streams = 4 hardware queues); rr_simulate_device, whose frames run on the
    // lanes' OWN streams beside the caller's stream, rotates over the first 3 only (same reason)
    int n_lanes = getenv("RR_LANES") ? atoi(getenv("RR_LANES")) : 4;
    n_lanes = std::max(1, std::min(n_lanes, 8));
    c->stream_lanes = getenv("RR_STREAM_LANES") ? std::max(1, std::min(atoi(getenv("RR_STREAM_LANES")), n_lanes))
                                                : std::min(3, n_lanes);
    if (getenv("RR_PASS0_AZ")) { const int a = atoi(getenv("RR_PASS0_AZ")); if (a == 1 || a == 2 || a == 4 || a == 8 || a == 16) c->pass0_az = a; }
    if (getenv("RR_STACK_LDS")) c->stack_lds_max = std::max(1, std::min(64, atoi(getenv("RR_STACK_LDS"))));
    if (getenv("RR_ROCTX") && atoi(getenv("RR_ROCTX")) != 0) c->roctx = roctx_load();
    if (getenv("RR_CULL_POP")) c->cull_pop = atoi(getenv("RR_CULL_POP")) != 0;
    if (getenv("RR_STACKLESS")) c->stackless = atoi(getenv("RR_STACKLESS")) != 0;
    if (getenv("RR_TRACE_CHUNK")) c->seg_chunk = std::max(0, std::min(1024, atoi(getenv("RR_TRACE_CHUNK"))));
    if (getenv("RR_GRAPHS")) c->use_graphs = atoi(getenv("RR_GRAPHS")) != 0;
    if (getenv("RR_HOST_SDMA")) c->host_sdma = atoi(getenv("RR_HOST_SDMA")) != 0;
    if (getenv("RR_TIGHT_GRID")) c->tight_grid = atoi(getenv("RR_TIGHT_GRID")) != 0;
    if (getenv("RR_METRICS_HIST")) c->metrics_hist = atoi(getenv("RR_METRICS_HIST")) != 0;
    if (getenv("RR_TIGHT_FORCE")) c->tight_force = std::max(0, atoi(getenv("RR_TIGHT_FORCE")));
    if (limit_of_same_material(c)) { g_create_error = "rr_create: device set-up failed"; rr_destroy(c); return nullptr; }
    c->lanes.resize((size_t)n_lanes);
    for (Lane& L : c->lanes) {
        if (hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&L.ev_ready, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.ev_consumed, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.slot[0].ev, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.slot[1].ev, hipEventDisableTiming) != hipSuccess) {
            g_create_error = "rr_create: lane stream/event creation failed"; rr_destroy(c); return nullptr;
        }
    }
    return c;
}

void rr_destroy(rr_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();   // frames may still be in flight on the lanes' or the caller's streams
    if (c->sdma) { sdma_destroy(c->sdma); c->sdma = nullptr; }      // (its queued copies wait for events that have completed by now)
    for (Delivery& d : c->deliveries) (void)hipEventDestroy(d.ev);
    for (hipEvent_t e : c->delivery_events) (void)hipEventDestroy(e);
    for (auto& kv : c->timers) for (auto& p : kv.second.pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    for (Lane& L : c->lanes) {
        if (L.stream) (void)hipStreamSynchronize(L.stream);
        if (L.h_hist) { (void)hipHostFree(L.h_hist); L.h_hist = nullptr; }
        drop_graphs(L);
        if (L.ev_ready) (void)hipEventDestroy(L.ev_ready);
        if (L.ev_consumed) (void)hipEventDestroy(L.ev_consumed);
        for (Delivery& d : L.slot) if (d.ev) (void)hipEventDestroy(d.ev);
        if (L.stream) (void)hipStreamDestroy(L.stream);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->h_frame) (void)hipHostFree(c->h_frame);
    if (c->h_rb) (void)hipHostFree(c->h_rb);
    delete c;      // frees every DevBuf of the context and its lanes: after their streams are gone, which is harmless on an idle device
}

const char* rr_last_error(const rr_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int rr_set_materials(rr_ctx* c, const rr_material* materials, size_t n_materials,
                     const int32_t* object_materials, size_t n_objects, int32_t material_id_air)
{
    if (!c) return -1;
    if (!materials || n_materials == 0) return fail(c, -3, "rr_set_materials: empty material table");
    if (n_objects && !object_materials) return fail(c, -3, "rr_set_materials: null object_materials");
    if (material_id_air < 0 || (size_t)material_id_air >= n_materials) return fail(c, -3, "rr_set_materials: material_id_air out of range");
    for (size_t i = 0; i < n_objects; i++)
        if (object_materials[i] < 0 || (size_t)object_materials[i] >= n_materials)
            return fail(c, -3, "rr_set_materials: object_materials entry out of range");
    if (c->have_materials && c->materials.size() == n_materials && c->object_materials.size() == n_objects &&
        c->material_id_air == material_id_air &&
        std::memcmp(c->materials.data(), materials, n_materials * sizeof(rr_material)) == 0 &&
        (n_objects == 0 || std::memcmp(c->object_materials.data(), object_materials, n_objects * sizeof(int32_t)) == 0))
        return 0;   // the per-frame loadParams() of the reference node, nothing new
    c->materials.assign(materials, materials + n_materials);
    c->object_materials.assign(object_materials, object_materials + n_objects);
    c->material_id_air = material_id_air;
    c->have_materials = true; c->tables_dirty |= rr_ctx::D_MAT;
    return 0;
}

int rr_set_config(rr_ctx* c, const rr_config* cfg)
{
    if (!c) return -1;
    if (!cfg) return fail(c, -3, "rr_set_config: null config");
    if (cfg->n_cells < 1 || cfg->n_cells > 8192) return fail(c, -3, "rr_set_config: n_cells must be in [1, 8192]");
    if (cfg->n_angles < 1 || cfg->n_angles > 65536) return fail(c, -3, "rr_set_config: n_angles must be in [1, 65536]");
    if (cfg->n_reflections < 0 || cfg->n_reflections > 16) return fail(c, -3, "rr_set_config: n_reflections must be in [0, 16]");
    if (cfg->signal_denoising < 0 || cfg->signal_denoising > 3) return fail(c, -3, "rr_set_config: signal_denoising must be 0..3");
    const int w = cfg->signal_denoising == 1 ? cfg->signal_denoising_triangular_width
                : cfg->signal_denoising == 2 ? cfg->signal_denoising_gaussian_width
                : cfg->signal_denoising == 3 ? cfg->signal_denoising_mb_width : 0;
    if (w < 0 || w > 256) return fail(c, -3, "rr_set_config: smear width must be in [0, 256]");
    if (cfg->ambient_noise < 0 || cfg->ambient_noise > 2) return fail(c, -3, "rr_set_config: ambient_noise must be 0..2");
    if (cfg->brdf_model < 0 || cfg->brdf_model > 1) return fail(c, -3, "rr_set_config: brdf_model must be 0 (A + B cos^C) or 1 (Cook-Torrance lobe)");
    if (!(cfg->resolution > 0.0)) return fail(c, -3, "rr_set_config: resolution must be > 0");
    // mode = (int)(fraction * width) indexes the weight table (RadarCPU.cpp:48-93): the reference's
    // sliders keep the fraction in [0, 1) (cfg/RadarModel.cfg:47-51); anything else would read outside it.
    // fraction * width < 1 (mode 0) is accepted and gives the reference's 0/0 weights
    const double mf = cfg->signal_denoising == 1 ? cfg->signal_denoising_triangular_mode
                    : cfg->signal_denoising == 2 ? cfg->signal_denoising_gaussian_mode
                    : cfg->signal_denoising == 3 ? cfg->signal_denoising_mb_mode : 0.0;
    if (!(mf >= 0.0 && mf < 1.0)) return fail(c, -3, "rr_set_config: denoising mode fraction must be in [0, 1)");
    // tfar of the ray cast; must stay far below the coordinate that marks an empty BVH child (3e38)
    if (!(cfg->range_max > 0.0f && cfg->range_max <= 1.0e30f)) return fail(c, -3, "rr_set_config: range_max must be in (0, 1e30]");
    if (!std::isfinite(cfg->wave_energy_threshold) || !std::isfinite(cfg->theta_min) || !std::isfinite(cfg->theta_inc))
        return fail(c, -3, "rr_set_config: non-finite wave_energy_threshold / theta_min / theta_inc");
    if (c->have_cfg && std::memcmp(&c->cfg, cfg, sizeof(rr_config)) == 0) return 0;
    c->cfg = *cfg;
    c->have_cfg = true; c->tables_dirty |= rr_ctx::D_CFG;
    return 0;
}

int rr_set_beam_samples(rr_ctx* c, const float* dirs, size_t n)
{
    if (!c) return -1;
    if (n && !dirs) return fail(c, -3, "rr_set_beam_samples: null dirs");
    if (n > 65536) return fail(c, -3, "rr_set_beam_samples: more than 65536 samples");
    for (size_t i = 0; i < 3 * n; i++) if (!std::isfinite(dirs[i])) return fail(c, -3, "rr_set_beam_samples: non-finite direction");
    if (c->beams.size() == 3 * n && (n == 0 || std::memcmp(c->beams.data(), dirs, 3 * n * sizeof(float)) == 0)) return 0;
    c->beams.assign(dirs, dirs + 3 * n);
    c->tables_dirty |= rr_ctx::D_BEAMS;
    return 0;
}

int rr_set_noise_offsets(rr_ctx* c, const float* rnd, size_t n)
{
    if (!c) return -1;
    if (n && !rnd) return fail(c, -3, "rr_set_noise_offsets: null pointer");
    for (size_t i = 0; i < n; i++) if (!std::isfinite(rnd[i])) return fail(c, -3, "rr_set_noise_offsets: non-finite offset");
    c->noise.assign(rnd, rnd + n);
    c->tables_dirty |= rr_ctx::D_NOISE;
    return 0;
}

int rr_set_motion_poses(rr_ctx* c, const float* poses, size_t n)
{
    if (!c) return -1;
    if (n && !poses) return fail(c, -3, "rr_set_motion_poses: null pointer");
    for (size_t i = 0; i < 7 * n; i++) if (!std::isfinite(poses[i])) return fail(c, -3, "rr_set_motion_poses: non-finite pose");
    c->motion.assign(poses, poses + 7 * n);
    c->tables_dirty |= rr_ctx::D_MOTION;
    return 0;
}

void* rr_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void rr_host_free(void* p) { if (p) (void)hipHostFree(p); }

int rr_synchronize(rr_ctx* c, void* stream)
{
    if (!c) return -1;
    RR_HIP(c, hipSetDevice(c->device));
    for (Lane& L : c->lanes) { const int rc = settle_lane(c, L); if (rc) return rc; }
    if (!c->deliveries.empty()) { const int rc = rr_wait_host(c, nullptr); if (rc) return rc; }
    for (Lane& L : c->lanes) RR_HIP(c, hipStreamSynchronize(L.stream));
    RR_HIP(c, hipStreamSynchronize(stream_of(c, stream)));
    // batches may run on OTHER caller streams as well (the header recommends four): a frame there could set a
    // bit between the read and the clear below, so the whole device is drained first -- after this call no
    // frame of this context is in flight anywhere and every error bit raised so far is reported exactly once
    RR_HIP(c, hipDeviceSynchronize());
    // error bits of every frame the asynchronous entry points enqueued since the last call (a frame that
    // overflowed its wave queue or met a bad material id is truncated, never silently)
    uint32_t bits = 0;
    for (Lane& L : c->lanes) {
        if (!L.d_sticky.p) continue;
        uint32_t b = 0;
        RR_HIP(c, hipMemcpy(&b, L.d_sticky.p, sizeof(b), hipMemcpyDeviceToHost));
        if (b) { bits |= b; RR_HIP(c, hipMemset(L.d_sticky.p, 0, sizeof(b))); }
    }
    return overflow_error(c, bits, true);
}

int rr_peek_error_bits_async(rr_ctx* c, uint32_t* h_bits, void* stream)
{
    if (!c) return -1;
    if (!h_bits) return fail(c, -3, "rr_peek_error_bits_async: null pointer");
    RR_HIP(c, hipSetDevice(c->device));
    Lane& L = c->lanes[c->last_lane];
    if (!L.d_sticky.p) { *h_bits = 0; return 0; }     // no frame has run on this lane yet
    hipStream_t s = stream_of(c, stream);
    if (host_visible(h_bits)) { launch_store_u32(L.d_sticky.p, h_bits, s); RR_HIP(c, hipGetLastError()); }     // (a kernel's store: no copy engine involved)
    else RR_HIP(c, hipMemcpyAsync(h_bits, L.d_sticky.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return 0;
}

}  // extern "C"
