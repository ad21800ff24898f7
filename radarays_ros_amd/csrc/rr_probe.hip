// rr_probe.hip -- what a context tells about its work: statistics, traversal shape, kernel timing, trace grid, launch-graph counts; the rr_debug_* hooks
#include "rr_ctx.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

extern "C" {

int rr_get_stats(rr_ctx* c, rr_stats* st)
{
    if (!c || !st) return -1;
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());
    std::memset(st, 0, sizeof(*st));
    Lane& L = c->lanes[c->last_lane];
    if (!L.d_counters.p) return 0;
    Counters h;
    { const int rcb = read_counters(c, h); if (rcb) return rcb; }
    st->nodes_visited = h.nodes; st->tris_tested = h.tris; st->overflow = h.overflow;
    if (getenv("RR_TRACE_STATS")) fprintf(stderr, "[rr stats] waves %u wave_iters %llu (avg %.1f) max_iters %u\n", h.n_waves, h.wave_iters, h.n_waves ? (double)h.wave_iters / h.n_waves : 0.0, h.max_iters);
    if (getenv("RR_TRACE_STATS") && h.n_waves)
        fprintf(stderr, "[rr stats] per wave: iterations %.2f, issuing node path %.2f, leaf path %.2f, live quad-steps %.1f (of 16 x iterations = %.1f)\n",
                (double)h.it_all / h.n_waves, (double)h.it_node / h.n_waves, (double)h.it_leaf / h.n_waves,
                (double)h.quad_steps / h.n_waves, 16.0 * h.it_all / h.n_waves);
    const size_t n = (size_t)L.last_n_seg * (size_t)L.last_n_passes;
    if (n && L.d_seg_stats.p) {
        std::vector<SegStats> ss(n);
        { const int rcb = read_back(c, ss.data(), L.d_seg_stats.p, n * sizeof(SegStats)); if (rcb) return rcb; }
        for (const SegStats& x : ss) { st->wave_passes += x.wave_passes; st->hits += x.hits; st->signals += x.signals; }
    }
    return 0;
}

int rr_set_stats_mode(rr_ctx* c, int enable) { if (!c) return -1; c->stats_mode = enable != 0; return 0; }

int rr_get_traversal_shape(rr_ctx* c, uint64_t out[8])
{
    if (!c || !out) return -1;
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());
    std::memset(out, 0, 8 * sizeof(uint64_t));
    Lane& L = c->lanes[c->last_lane];
    if (!L.d_counters.p) return 0;
    Counters h;
    { const int rcb = read_counters(c, h); if (rcb) return rcb; }
    out[0] = h.n_waves; out[1] = h.it_all; out[2] = h.it_node; out[3] = h.it_leaf; out[4] = h.quad_steps; out[5] = h.max_iters;
    out[6] = h.nodes; out[7] = h.quad_steps > h.nodes ? h.quad_steps - h.nodes : 0;
    return 0;
}
int rr_set_timing_mode(rr_ctx* c, int enable) { if (!c) return -1; c->timing = enable; return 0; }

int rr_get_kernel_time(rr_ctx* c, const char* kernel, double* total_ms, uint64_t* launches, int reset)
{
    if (!c || !kernel) return -1;
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());
    KernelTimer& t = c->timers[kernel];
    for (auto& p : t.pending) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) { t.total_ms += ms; t.launches++; t.samples_ms.push_back(ms); }
        c->event_pool.push_back(p.first); c->event_pool.push_back(p.second);
    }
    t.pending.clear();
    if (total_ms) *total_ms = t.total_ms;
    if (launches) *launches = t.launches;
    if (reset) { t.total_ms = 0.0; t.launches = 0; t.samples_ms.clear(); }
    return 0;
}

int rr_get_kernel_samples(rr_ctx* c, const char* kernel, float* out_ms, size_t capacity, size_t* n_out)
{
    if (!c || !kernel || !n_out) return -1;
    int rc = rr_get_kernel_time(c, kernel, nullptr, nullptr, 0); if (rc) return rc;
    const KernelTimer& t = c->timers[kernel];
    *n_out = t.samples_ms.size();
    if (out_ms) for (size_t i = 0; i < t.samples_ms.size() && i < capacity; i++) out_ms[i] = t.samples_ms[i];
    return 0;
}

int rr_reserve_timing_events(rr_ctx* c, size_t n)
{
    if (!c) return -1;
    RR_HIP(c, hipSetDevice(c->device));
    while (c->event_pool.size() < n) { hipEvent_t e = nullptr; RR_HIP(c, hipEventCreate(&e)); c->event_pool.push_back(e); }
    return 0;
}

int rr_get_trace_grid(rr_ctx* c, uint32_t out_rows[24], uint32_t out_hist[24], uint64_t* repaired_groups)
{
    if (!c) return -1;
    static_assert(kMaxPasses == 24, "rr_get_trace_grid's arrays");
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, hipDeviceSynchronize());
    const Lane& L = c->lanes[c->last_lane];
    uint64_t rep = 0;
    for (int k = 0; k < kMaxPasses; k++) { if (out_rows) out_rows[k] = L.last_rows[k]; if (out_hist) out_hist[k] = 0; }
    for (const Lane& o : c->lanes) {
        if (!o.d_hint.p || o.hist_gen != c->hist_gen) continue;
        GridHint h;
        RR_HIP(c, hipMemcpy(&h, o.d_hint.p, sizeof(h), hipMemcpyDeviceToHost));
        rep += h.repaired;
        for (int k = 0; k < kMaxPasses && out_hist; k++) out_hist[k] = std::max(out_hist[k], h.hist[k]);
    }
    if (repaired_groups) *repaired_groups = rep;
    return 0;
}

int rr_get_graph_stats(rr_ctx* c, uint64_t* captures, uint64_t* replays)
{
    if (!c) return -1;
    if (captures) *captures = c->graph_captures;
    if (replays) *replays = c->graph_replays;
    return 0;
}

int rr_debug_fresnel(rr_ctx* c, size_t n, const float* normals, const float* dirs, const double* energy, const double* v1, const float* v2,
                     float* out_refl_dir, double* out_refl_energy, float* out_refr_dir, double* out_refr_energy)
{
    if (!c) return -1;
    if (n == 0) return 0;
    if (!normals || !dirs || !energy || !v1 || !v2 || !out_refl_dir || !out_refl_energy || !out_refr_dir || !out_refr_energy)
        return fail(c, -3, "rr_debug_fresnel: null pointer");
    RR_HIP(c, hipSetDevice(c->device));
    DevBuf<float> d_n, d_d, d_v2, d_rd, d_td; DevBuf<double> d_e, d_v1, d_re, d_te;
    RR_HIP(c, d_n.ensure(3 * n)); RR_HIP(c, d_d.ensure(3 * n)); RR_HIP(c, d_v2.ensure(n)); RR_HIP(c, d_rd.ensure(3 * n)); RR_HIP(c, d_td.ensure(3 * n));
    RR_HIP(c, d_e.ensure(n)); RR_HIP(c, d_v1.ensure(n)); RR_HIP(c, d_re.ensure(n)); RR_HIP(c, d_te.ensure(n));
    RR_HIP(c, hipMemcpy(d_n.p, normals, 3 * n * sizeof(float), hipMemcpyHostToDevice));
    RR_HIP(c, hipMemcpy(d_d.p, dirs, 3 * n * sizeof(float), hipMemcpyHostToDevice));
    RR_HIP(c, hipMemcpy(d_v2.p, v2, n * sizeof(float), hipMemcpyHostToDevice));
    RR_HIP(c, hipMemcpy(d_e.p, energy, n * sizeof(double), hipMemcpyHostToDevice));
    RR_HIP(c, hipMemcpy(d_v1.p, v1, n * sizeof(double), hipMemcpyHostToDevice));
    launch_debug_fresnel(n, d_n.p, d_d.p, d_e.p, d_v1.p, d_v2.p, d_rd.p, d_re.p, d_td.p, d_te.p, c->stream);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipStreamSynchronize(c->stream));
    RR_HIP(c, hipMemcpy(out_refl_dir, d_rd.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    RR_HIP(c, hipMemcpy(out_refr_dir, d_td.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    RR_HIP(c, hipMemcpy(out_refl_energy, d_re.p, n * sizeof(double), hipMemcpyDeviceToHost));
    RR_HIP(c, hipMemcpy(out_refr_energy, d_te.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int rr_debug_brdf(rr_ctx* c, size_t n, const float* in5, int brdf_model, float* out)
{
    if (!c) return -1;
    if (n == 0) return 0;
    if (!in5 || !out) return fail(c, -3, "rr_debug_brdf: null pointer");
    if (brdf_model != 0 && brdf_model != 1) return fail(c, -3, "rr_debug_brdf: brdf_model must be 0 or 1");
    RR_HIP(c, hipSetDevice(c->device));
    DevBuf<float> d_in, d_out;
    RR_HIP(c, d_in.ensure(5 * n));
    RR_HIP(c, d_out.ensure(n));
    RR_HIP(c, hipMemcpy(d_in.p, in5, 5 * n * sizeof(float), hipMemcpyHostToDevice));
    launch_debug_brdf(n, d_in.p, brdf_model, d_out.p, c->stream);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipStreamSynchronize(c->stream));
    RR_HIP(c, hipMemcpy(out, d_out.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

int rr_debug_column(rr_ctx* c, int n_frames, int n_loc, int az_begin, int n_passes, int n_beam, int record_multi_path,
                    const rr_echo* list, const uint32_t* list_count, size_t list_stride,
                    const rr_echo* slots, const uint8_t* slot_hit, const uint32_t* slot_count, size_t slot_stride,
                    float* out_f32, uint8_t* out_u8, uint32_t* out_stats)
{
    static_assert(sizeof(rr_echo) == sizeof(SigRec) && sizeof(SegStats) == 16, "rr_debug_column copies records as they lie");
    if (!c) return -1;
    if (!c->have_cfg) return fail(c, -2, "rr_set_config has not been called");
    const rr_config& g = c->cfg;
    if (n_frames < 1 || n_frames > RR_MAX_BATCH) return fail(c, -3, "rr_debug_column: n_frames must be 1..64");
    if (n_loc < 1 || az_begin < 0 || az_begin > g.n_angles - n_loc) return fail(c, -3, "rr_debug_column: azimuth block out of bounds");
    if (n_passes < 1 || n_passes > std::max(1, g.n_reflections))
        return fail(c, -3, "rr_debug_column: n_passes must be in [1, max(1, n_reflections)]: the lane's buffers are sized by the config");
    if (n_beam < 0) return fail(c, -3, "rr_debug_column: negative n_beam");
    if (!out_u8) return fail(c, -3, "rr_debug_column: null output");
    const bool use_list = n_passes > 1 && list_stride > 0, use_slots = slot_stride > 0;
    if ((use_list && (!list || !list_count)) || (use_slots && (!slots || !slot_hit)) || (use_slots && n_passes > 1 && !slot_count))
        return fail(c, -3, "rr_debug_column: null stream");
    RR_HIP(c, hipSetDevice(c->device));
    int rc = upload_tables(c); if (rc) return rc;
    const int n_seg = n_frames * n_loc;
    const size_t S = (size_t)n_seg;
    Lane& L = c->lanes[0];
    rc = take_lane(c, 0, c->stream); if (rc) return rc;
    rc = prepare_lane(c, L, n_seg, true); if (rc) return rc;
    // what the lane's buffers cannot hold is refused before anything is written
    const size_t cap = (size_t)L.buf_cap, sigcap = (size_t)L.buf_sigcap;
    if ((size_t)n_beam > cap) return fail(c, -3, "rr_debug_column: n_beam exceeds the lane's wave capacity");
    if (use_list && list_stride > sigcap) return fail(c, -3, "rr_debug_column: list_stride exceeds the lane's signal capacity");
    if (use_slots && slot_stride > cap) return fail(c, -3, "rr_debug_column: slot_stride exceeds the lane's wave capacity");
    if (n_passes == 1 && (size_t)n_beam > slot_stride) return fail(c, -3, "rr_debug_column: one pass stages n_beam waves per segment, more than slot_stride");
    for (size_t s = 0; s < S; s++) {
        if (n_passes > 1 && list_count && list_count[s] > list_stride) return fail(c, -3, "rr_debug_column: a list count exceeds list_stride");
        if (n_passes > 1 && slot_count && slot_count[s] > slot_stride) return fail(c, -3, "rr_debug_column: a slot count exceeds slot_stride");
    }
    // the two stream forms as the frame path leaves them: sig / sig_count, and sigtmp / cflag bit 2 / count of the last pass
    hipStream_t st = c->stream;
    std::vector<uint32_t> zeros(S, 0u);
    const int last = (n_passes - 1) & 1;
    RR_HIP(c, hipMemcpyAsync(L.d_sig_count.p, use_list ? list_count : zeros.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    RR_HIP(c, hipMemcpyAsync(L.d_count[last].p, (use_slots && n_passes > 1) ? slot_count : zeros.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (use_list)
        RR_HIP(c, hipMemcpy2DAsync(L.d_sig.p, sigcap * sizeof(SigRec), list, list_stride * sizeof(rr_echo), list_stride * sizeof(rr_echo), S, hipMemcpyHostToDevice, st));
    std::vector<uint8_t> flags;
    if (use_slots) {
        RR_HIP(c, hipMemcpy2DAsync(L.d_sigtmp.p, 2 * cap * sizeof(SigRec), slots, 2 * slot_stride * sizeof(rr_echo), 2 * slot_stride * sizeof(rr_echo), S,
                                   hipMemcpyHostToDevice, st));
        flags.assign(S * 2 * slot_stride, 0);
        for (size_t k = 0; k < S * slot_stride; k++) flags[2 * k] = slot_hit[k] ? 4 : 0;      // bit 2, even slot
        RR_HIP(c, hipMemcpy2DAsync(L.d_cflag.p, 2 * cap, flags.data(), 2 * slot_stride, 2 * slot_stride, S, hipMemcpyHostToDevice, st));
    }
    Params P; std::memset(&P, 0, sizeof(P));
    P.smear = c->d_smear.p; P.signal_denoising = c->smear.empty() ? 0 : g.signal_denoising;
    P.smear_w = (int)c->smear.size(); P.smear_mode = c->smear_mode;
    P.noise_rnd = g.ambient_noise ? c->d_noise.p : nullptr; P.noise_rows = c->noise_rows; P.decay = c->d_decay.p;
    P.count[0] = L.d_count[0].p; P.count[1] = L.d_count[1].p;
    P.cflag = L.d_cflag.p; P.sigtmp = L.d_sigtmp.p; P.sig = L.d_sig.p; P.sig_count = L.d_sig_count.p; P.seg_stats = L.d_seg_stats.p;
    P.cols_u8 = L.d_cols_u8.p; P.cols_f32 = L.d_cols_f32.p;
    P.az_begin = az_begin; P.n_seg = n_seg; P.n_loc = n_loc; P.n_frames = n_frames;
    P.n_beam = n_beam; P.cap = L.buf_cap; P.sigcap = L.buf_sigcap;
    P.n_cells = g.n_cells; P.n_angles = g.n_angles;
    P.n_passes = n_passes; P.record_multi_path = record_multi_path != 0;
    P.ambient_noise = g.ambient_noise; P.scroll = g.scroll_image;
    P.resolution = g.resolution; P.energy_max_f = (float)g.energy_max; P.signal_max = g.signal_max;
    P.noise_at_0 = g.ambient_noise_at_signal_0; P.noise_at_1 = g.ambient_noise_at_signal_1;
    P.noise_e_max = g.ambient_noise_energy_max; P.noise_e_min = g.ambient_noise_energy_min; P.noise_e_loss = g.ambient_noise_energy_loss;
    L.last_n_seg = 0; L.last_n_passes = 0;       // (no frame: rr_get_stats has nothing to add up on this lane)
    launch_column(P, st);
    RR_HIP(c, hipGetLastError());
    const size_t px = S * (size_t)g.n_cells;
    std::vector<SegStats> ss(out_stats ? S : 0);
    RR_HIP(c, hipMemcpyAsync(out_u8, L.d_cols_u8.p, px, hipMemcpyDeviceToHost, st));
    if (out_f32) RR_HIP(c, hipMemcpyAsync(out_f32, L.d_cols_f32.p, px * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_stats) RR_HIP(c, hipMemcpyAsync(ss.data(), L.d_seg_stats.p + (size_t)(n_passes - 1) * S, S * sizeof(SegStats), hipMemcpyDeviceToHost, st));
    RR_HIP(c, give_lane(L, st));
    RR_HIP(c, hipStreamSynchronize(st));
    for (size_t s = 0; s < ss.size(); s++) { out_stats[3 * s] = ss[s].wave_passes; out_stats[3 * s + 1] = ss[s].hits; out_stats[3 * s + 2] = ss[s].signals; }
    return 0;
}

int rr_debug_trace(rr_ctx* c, const float* origs, const float* dirs, size_t n, float* out_t, uint32_t* out_face)
{
    if (!c) return -1;
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    if (n == 0) return 0;
    if (!origs || !dirs || !out_t || !out_face) return fail(c, -3, "rr_debug_trace: null pointer");
    RR_HIP(c, hipSetDevice(c->device));
    const size_t chunk = 1u << 16;
    const int stack_lds = (int)std::max<uint32_t>(1, std::min<uint32_t>(c->stack_need, (uint32_t)c->stack_lds_max));
    const int spill_depth = (int)c->stack_need - stack_lds;
    DevBuf<float> d_o, d_d, d_t; DevBuf<uint32_t> d_f, d_spill;
    RR_HIP(c, d_o.ensure(3 * chunk)); RR_HIP(c, d_d.ensure(3 * chunk)); RR_HIP(c, d_t.ensure(chunk));
    RR_HIP(c, d_f.ensure(chunk)); RR_HIP(c, d_spill.ensure(spill_depth > 0 ? (size_t)spill_depth * chunk : 1));
    Params P; std::memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const Node4*>(c->d_bvh.p); P.tris = reinterpret_cast<const TriRec*>(c->d_bvh.p + c->tri_base4);
    P.tri_base4 = c->tri_base4; P.range_max = c->have_cfg ? c->cfg.range_max : 1000.0f; P.hit_pad = c->hit_pad;
    P.spill = d_spill.p; P.spill_stride = (int)chunk; P.stack_lds = stack_lds; P.spill_depth = std::max(0, spill_depth);
    P.cull_pop = c->cull_pop;
    for (size_t b = 0; b < n; b += chunk) {
        const size_t m = std::min(chunk, n - b);
        RR_HIP(c, hipMemcpy(d_o.p, origs + 3 * b, 3 * m * sizeof(float), hipMemcpyHostToDevice));
        RR_HIP(c, hipMemcpy(d_d.p, dirs + 3 * b, 3 * m * sizeof(float), hipMemcpyHostToDevice));
        launch_debug_trace(P, d_o.p, d_d.p, (int)m, d_t.p, d_f.p, c->stream);
        RR_HIP(c, hipStreamSynchronize(c->stream));
        RR_HIP(c, hipMemcpy(out_t + b, d_t.p, m * sizeof(float), hipMemcpyDeviceToHost));
        RR_HIP(c, hipMemcpy(out_face + b, d_f.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return 0;
}

}  // extern "C"
