// rr_probe.hip -- what a context tells about its work: statistics, traversal shape, kernel timing, trace grid, launch-graph counts; the rr_debug_* hooks
#include "rr_ctx.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>

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
