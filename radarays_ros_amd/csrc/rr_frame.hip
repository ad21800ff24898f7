// rr_frame.hip -- a frame on a lane: the lane's buffers and its hand-over, run_frame (the launch chain of a batch and its launch-graph
// cache), the plain rr_simulate*_device / rr_assemble_*_device entry points, the synchronous rr_simulate, the delivery of images to host
// memory.  The entry points of the side chains (provenance, wave paths, Doppler) are in rr_side.hip.
#include "rr_ctx.h"
#include "rr_hostprof.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <vector>

namespace rr {
namespace {

// number of ray-cast passes the frame buffers and the launch loop are sized for: the config's, or the largest of a
// parameter batch while rr_simulate_param_sets_device assembles it
inline int eff_passes(const rr_ctx* c) { return c->passes_override >= 0 ? c->passes_override : c->cfg.n_reflections; }
inline rr_config eff_config(const rr_ctx* c) { rr_config g = c->cfg; g.n_reflections = eff_passes(c); return g; }

int wave_capacity(const rr_config& cfg, int n_beam)
{
    long cap = cfg.max_waves_per_azimuth;
    if (cap <= 0) {
        cap = n_beam;
        for (int p = 1; p < cfg.n_reflections && cap < 65536; p++) cap *= 2;
        cap = std::min<long>(cap, 65536);
    }
    cap = std::max<long>(cap, n_beam);
    return (int)cap;
}

int signal_capacity(const rr_config& cfg, int n_beam, int cap)
{
    long tot = 0, w = n_beam;
    for (int p = 0; p < cfg.n_reflections; p++) { tot += std::min<long>(w, cap); w = std::min<long>(2 * w, cap); }
    if (cfg.record_multi_path) tot *= 2;
    return (int)std::max<long>(tot, 1);
}

void drop_graph(Lane::FrameGraph& fg)
{
    for (int k = 0; k < 2; k++) {       // an exec is destroyed only after its last launch has left the GPU
        if (fg.ev[k]) { if (fg.ev_pending[k]) (void)hipEventSynchronize(fg.ev[k]); (void)hipEventDestroy(fg.ev[k]); fg.ev[k] = nullptr; fg.ev_pending[k] = false; }
    }
    if (fg.ge) (void)hipGraphExecDestroy(fg.ge);
    if (fg.ge2) (void)hipGraphExecDestroy(fg.ge2);
    if (fg.g) (void)hipGraphDestroy(fg.g);
    fg.ge = fg.ge2 = nullptr; fg.g = nullptr;
}
int ensure_frame_buffers(rr_ctx* c, Lane& L, int n_seg, bool want_f32)
{
    const rr_config g = eff_config(c);      // (a parameter batch may ask for more passes than the config)
    const int n_beam = (int)(c->beams.size() / 3);
    const int cap = wave_capacity(g, n_beam);
    const int sigcap = signal_capacity(g, n_beam, cap);
    const size_t S = (size_t)n_seg;
    const size_t per_seg = (size_t)cap * (2 * 2 * 48 + 2 * 4 + 2 * 9 + 8 + 8) + (size_t)sigcap * 8 + (size_t)g.n_cells * 5;
    size_t free_b = 0, total_b = 0;
    RR_HIP(c, hipMemGetInfo(&free_b, &total_b));
    if (S * per_seg > total_b / 2)
        return fail(c, -6, "wave queue capacity needs more than half of device memory; lower max_waves_per_azimuth");
    for (int k = 0; k < 2; k++) {
        RR_HIP(c, L.d_wA[k].ensure(S * 2 * cap));
        RR_HIP(c, L.d_wB[k].ensure(S * 2 * cap));
        RR_HIP(c, L.d_wC[k].ensure(S * 2 * cap));
        RR_HIP(c, L.d_idx[k].ensure(S * cap));
        RR_HIP(c, L.d_torder[k].ensure(S * cap));
        RR_HIP(c, L.d_count[k].ensure(S));
    }
    RR_HIP(c, L.d_cflag.ensure(S * 2 * cap));
    RR_HIP(c, L.d_refpos.ensure(S * 2 * cap));
    RR_HIP(c, L.d_sorder.ensure(S * cap));
    RR_HIP(c, L.d_n_air.ensure(S));
    RR_HIP(c, L.d_sigtmp.ensure(S * 2 * cap));
    RR_HIP(c, L.d_hit.ensure(S * cap));
    RR_HIP(c, L.d_sig.ensure(S * sigcap));
    RR_HIP(c, L.d_sig_count.ensure(S));
    if (!L.d_counters.p) { RR_HIP(c, L.d_counters.ensure(1)); RR_HIP(c, hipMemset(L.d_counters.p, 0, sizeof(Counters))); }
    if (!L.d_sticky.p) { RR_HIP(c, L.d_sticky.ensure(1)); RR_HIP(c, hipMemset(L.d_sticky.p, 0, sizeof(uint32_t))); }
    RR_HIP(c, L.d_seg_stats.ensure(S * (size_t)std::max(1, g.n_reflections)));
    if (!L.d_hint.p) { RR_HIP(c, L.d_hint.ensure(1)); RR_HIP(c, hipMemset(L.d_hint.p, 0, sizeof(GridHint))); L.hist_gen = 0; }
    if (!L.h_hist) { RR_HIP(c, hipHostMalloc((void**)&L.h_hist, kMaxPasses * sizeof(uint32_t), hipHostMallocDefault)); std::memset(L.h_hist, 0, kMaxPasses * sizeof(uint32_t)); }
    RR_HIP(c, L.d_ovf_list.ensure(S * (size_t)kMaxPasses)); L.ovf_stride = (int)S;
    RR_HIP(c, L.d_cols_u8.ensure(S * g.n_cells));
    if (want_f32) RR_HIP(c, L.d_cols_f32.ensure(S * g.n_cells));
    // traversal stack: LDS part + spill
    L.stack_lds = (int)std::max<uint32_t>(1, std::min<uint32_t>(c->stack_need, (uint32_t)c->stack_lds_max));   // 64 B of LDS per entry per wave
    const int spill_depth = (int)c->stack_need - L.stack_lds;
    // one spill column per ray slot a launch can address: later passes ceil(cap/32)*32 slots per segment,
    // pass 0 its (sample x azimuth) tiles, whose padding can exceed S * n_beam (e.g. ONE segment: 16 x n_beam)
    const size_t A0 = (size_t)c->pass0_az, Sw0 = 16 / A0;
    const size_t slots0 = ((((S + A0 - 1) / A0) * (((size_t)n_beam + Sw0 - 1) / Sw0) + 1) / 2) * 32;      // (rounded up to pairs of waves: covers 64- and 128-thread workgroups)
    const size_t threads = std::max(S * (size_t)((cap + 63) / 64) * 64, slots0);
    L.spill_stride = (int)threads;
    if (spill_depth > 0) RR_HIP(c, L.d_spill.ensure((size_t)spill_depth * threads));
    else RR_HIP(c, L.d_spill.ensure(1));
    L.buf_seg = n_seg; L.buf_cap = cap; L.buf_sigcap = sigcap; L.buf_cells = g.n_cells; L.buf_passes = std::max(1, g.n_reflections);
    RR_HIP(c, L.d_poses.ensure((size_t)RR_MAX_BATCH * 8));
    L.graph_gen = 0;           // the lane's buffers moved: its captured launches point at the old ones
    return 0;
}

void fill_params(rr_ctx* c, Lane& L, Params& P, const float pose[7], int az_begin, int n_seg,
                 uint8_t* d_cols_u8, float* d_cols_f32)
{
    const rr_config g = eff_config(c);      // (a parameter batch may ask for more passes than the config)
    std::memset(&P, 0, sizeof(P));
    P.nodes = reinterpret_cast<const Node4*>(c->d_bvh.p); P.tris = reinterpret_cast<const TriRec*>(c->d_bvh.p + c->tri_base4);
    P.tri_base4 = c->tri_base4;
    P.q_as = c->d_qas.p; P.beams = c->d_beams.p; P.beam_order = c->d_beam_order.p; P.beam_order2 = c->d_beam_order2.p; P.materials = c->d_materials.p;
    P.mat_limits = c->d_mat_limits.p; P.limit_same = c->limit_same;
    P.object_materials = c->d_objmat.p; P.smear = c->d_smear.p;
    P.noise_rnd = g.ambient_noise ? c->d_noise.p : nullptr; P.noise_rows = c->noise_rows;
    P.decay = c->d_decay.p;
    P.motion_poses = c->motion.empty() ? nullptr : c->d_motion.p; P.motion_rows = c->motion_rows;
    for (int k = 0; k < 2; k++) {
        P.waves[k].A = L.d_wA[k].p; P.waves[k].B = L.d_wB[k].p; P.waves[k].C = L.d_wC[k].p;
        P.idx[k] = L.d_idx[k].p; P.count[k] = L.d_count[k].p; P.torder[k] = L.d_torder[k].p;
    }
    P.refpos = L.d_refpos.p; P.sorder = L.d_sorder.p; P.n_air = L.d_n_air.p;
    P.cflag = L.d_cflag.p; P.sigtmp = L.d_sigtmp.p; P.hit = L.d_hit.p;
    P.sig = L.d_sig.p; P.sig_count = L.d_sig_count.p; P.spill = L.d_spill.p; P.counters = L.d_counters.p; P.sticky = L.d_sticky.p; P.seg_stats = L.d_seg_stats.p;
    P.cols_u8 = d_cols_u8; P.cols_f32 = d_cols_f32;
    P.az_begin = az_begin; P.n_seg = n_seg;
    P.n_beam = (int)(c->beams.size() / 3); P.cap = L.buf_cap; P.sigcap = L.buf_sigcap;
    P.n_cells = g.n_cells; P.n_angles = g.n_angles;
    P.n_materials = (int)c->materials.size(); P.n_objects = (int)c->object_materials.size();
    P.material_id_air = c->material_id_air;
    P.n_passes = g.n_reflections;
    P.record_multi_reflection = g.record_multi_reflection; P.record_multi_path = g.record_multi_path;
    P.brdf_model = g.brdf_model;
    P.signal_denoising = c->smear.empty() ? 0 : g.signal_denoising;
    P.smear_w = (int)c->smear.size(); P.smear_mode = c->smear_mode;
    P.ambient_noise = g.ambient_noise; P.scroll = g.scroll_image;
    P.thr = g.wave_energy_threshold; P.range_max = g.range_max; P.hit_pad = c->hit_pad;
    P.resolution = g.resolution; P.multipath_threshold = g.multipath_threshold;
    P.energy_max_f = (float)g.energy_max; P.signal_max = g.signal_max;
    P.noise_at_0 = g.ambient_noise_at_signal_0; P.noise_at_1 = g.ambient_noise_at_signal_1;
    P.noise_e_max = g.ambient_noise_energy_max; P.noise_e_min = g.ambient_noise_energy_min;
    P.noise_e_loss = g.ambient_noise_energy_loss;
    P.spill_stride = L.spill_stride; P.stack_lds = L.stack_lds;
    P.spill_depth = std::max(0, (int)c->stack_need - L.stack_lds);
    P.pass0_az = c->pass0_az;
    P.cull_pop = c->cull_pop; P.seg_chunk = c->seg_chunk; P.stackless = c->stackless;
    P.grid_hint = L.d_hint.p; P.ovf_list = L.d_ovf_list.p; P.ovf_stride = L.ovf_stride;     // rows stay at the bound until run_frame tightens them
    P.hist_host = (c->tight_grid && g.n_reflections > 1) ? L.h_hist : nullptr;              // the chain's k_column stores the history there (read without a fence by later batches)
}

// The lane's running state of a paths chain for its current frame buffers (after prepare_lane): 16 bytes per segment
int ensure_path_state(rr_ctx* c, Lane& L)
{
    if (L.d_path_state.p && L.path_seg >= L.buf_seg) return 0;
    RR_HIP(c, hipDeviceSynchronize());      // a paths chain in flight may still use the old buffer
    RR_HIP(c, L.d_path_state.ensure((size_t)L.buf_seg));
    L.path_seg = L.buf_seg;
    return 0;
}

// The lane's Doppler buffers for its current frame and provenance buffers (after prepare_lane and ensure_prov_buffers): 32 bytes of
// state per wave and pass parity, 16 bytes per echo of the lists, and the small arrays of the list-only column launch
int ensure_dop_buffers(rr_ctx* c, Lane& L, bool want_vel)
{
    const size_t S = (size_t)L.buf_seg, n_in = 64 + 2 * (size_t)c->n_objects;
    const bool fits = L.d_dop_state.p && L.dop_seg >= L.buf_seg && L.dop_cap == L.buf_cap && L.dop_echo_cap == L.prov_cap && L.dop_cells == L.buf_cells &&
                      L.dop_obj >= n_in && (!want_vel || (L.d_dop_vel_cols.p && L.d_dop_vel_cols.n >= S * (size_t)L.buf_cells));
    if (fits) return 0;
    size_t free_b = 0, total_b = 0;
    RR_HIP(c, hipMemGetInfo(&free_b, &total_b));
    if (S * ((size_t)L.buf_cap * 64 + (size_t)L.prov_cap * 16 + (size_t)L.buf_cells * 4) > total_b / 2)
        return fail(c, -6, "the wave states and echo lists of a Doppler call need more than half of device memory; fewer frames per call or a lower max_waves_per_azimuth");
    RR_HIP(c, hipDeviceSynchronize());      // a Doppler chain in flight may still use the old buffers
    RR_HIP(c, L.d_dop_state.ensure(2 * S * (size_t)L.buf_cap * 2));
    RR_HIP(c, L.d_dop_rate.ensure(S * (size_t)L.prov_cap));
    RR_HIP(c, L.d_dop_sig.ensure(S * (size_t)L.prov_cap));
    RR_HIP(c, L.d_dop_count.ensure(S));
    RR_HIP(c, L.d_dop_zero.ensure(S));
    RR_HIP(c, hipMemset(L.d_dop_zero.p, 0, S * sizeof(uint32_t)));
    RR_HIP(c, L.d_dop_stats.ensure(2 * S));
    RR_HIP(c, L.d_dop_in.ensure(n_in));
    if (want_vel) RR_HIP(c, L.d_dop_vel_cols.ensure(S * (size_t)L.buf_cells));
    L.dop_seg = L.buf_seg; L.dop_cap = L.buf_cap; L.dop_echo_cap = L.prov_cap; L.dop_cells = L.buf_cells; L.dop_obj = n_in;
    return 0;
}

// device -> host on stream s: the library's own copy kernel (8 workgroups, all on XCD 0) when the destination is page-locked
// (`visible`) and everything is 16-byte aligned, else hipMemcpyAsync (rr_copy_to_host_async in the header says why)
int copy_out(rr_ctx* c, const void* d_src, void* h_dst, size_t bytes, bool visible, hipStream_t s)
{
    if (bytes == 0) return 0;
    if (visible && bytes % 16 == 0 && ((uintptr_t)h_dst | (uintptr_t)d_src) % 16 == 0) {
        launch_copy_host(d_src, h_dst, bytes, 8, 0, s);
        RR_HIP(c, hipGetLastError());
    } else RR_HIP(c, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, s));
    return 0;
}

// the delivery has left (host wait): its SDMA job has completed, or else the event behind its stream-ordered copy
int wait_delivery(rr_ctx* c, Delivery& d)
{
    if (!d.dst) return 0;
    if (d.job) sdma_wait(c->sdma, d.job);
    else RR_HIP(c, hipEventSynchronize(d.ev));
    d.dst = nullptr; d.job = 0;
    return 0;
}

// the SDMA worker of the context, made on first use (nullptr: not available / switched off)
SdmaCopier* sdma_of(rr_ctx* c, const void* any_device_ptr)
{
    if (!c->host_sdma) return nullptr;
    if (!c->sdma && !c->sdma_tried) {
        c->sdma_tried = true;
        std::string why;
        c->sdma = sdma_create(c->device, any_device_ptr, why);
        if (!c->sdma && getenv("RR_HOST_SDMA_VERBOSE")) fprintf(stderr, "[rr] SDMA delivery not available: %s\n", why.c_str());
    }
    if (c->sdma && sdma_failed(c->sdma, nullptr)) {
        if (getenv("RR_HOST_SDMA_VERBOSE")) { std::string why; (void)sdma_failed(c->sdma, &why); fprintf(stderr, "[rr] SDMA delivery switched off: %s\n", why.c_str()); }
        c->host_sdma = 0;
        return nullptr;
    }
    return c->sdma;
}

// later-pass trace rows as long as earlier batches needed (rr_device.h: GridHint).  Not for the statistics build (the
// repair launch does not count), the spill path (its columns are laid out for the full rows) or parameter batches
// (frames with their own beams and passes)
int choose_trace_rows(rr_ctx* c, Lane& L, Params& P, const rr_config& g, hipStream_t s)
{
    if (L.hist_gen != c->hist_gen) {
        RR_HIP(c, hipMemsetAsync(L.d_hint.p, 0, sizeof(GridHint), s));
        std::memset(L.h_hist, 0, kMaxPasses * sizeof(uint32_t));
        L.hist_gen = c->hist_gen;
    }
    const bool tight = c->tight_grid && !c->stats_mode && !P.set_mode && P.spill_depth == 0 && g.n_reflections <= kMaxPasses;
    if (tight) {
        for (int pass = 1; pass < g.n_reflections; pass++) {
            const long bound = std::min<long>((long)P.cap, pass < 20 ? (long)P.n_beam << pass : (long)P.cap);
            const long full = (bound + 15) / 16;
            uint32_t h = 0;
            for (const Lane& o : c->lanes) if (o.h_hist && o.hist_gen == c->hist_gen) h = std::max(h, o.h_hist[pass]);
            long row = h ? std::min<long>(full, ((long)h + (long)h / 16 + 32 + 15) / 16) : full;
            // an ODD number of workgroups per row: the hardware deals workgroups out to the 8 XCDs round robin in flat order
            // (y * row + x), so with a row length that shares a factor with 8 the same x always lands on the same XCDs -- and the
            // tail of every row (few or no live rays) always on the same ones.  Rows rounded to a multiple of four: 435 -> 457 us
            // per launch alone, -2.4 % images/s on the target (measured by accident, DESIGN_EXPERIMENTS.md)
            row |= 1;
            if (c->tight_force) row = std::min<long>(full, c->tight_force);
            P.tight_groups[pass] = (row < full && row < 65535) ? (unsigned short)row : 0;
        }
    }
    std::memcpy(L.last_rows, P.tight_groups, sizeof(L.last_rows));
    return 0;
}

// what a side chain adds to the launch chain, filled in by run_frame: the wave rows; the Doppler arguments and Q as the list-only column launch reads it
struct ChainSide { const WaveOut* wo = nullptr; const DopArgs* da = nullptr; const Params* Qlist = nullptr; };

// the launch chain of the batch
int issue_chain(rr_ctx* c, const Params& Q, const PoseArgs& pa, const rr_config& g, hipStream_t s, const ChainSide& side = {})
{
    const WaveOut* wo = side.wo; const DopArgs* da = side.da;
    for (int pass = 0; pass < g.n_reflections; pass++) {
        if (c->roctx) roctx_push(pass == 0 ? "trace pass 0" : "trace");
        if (c->timing) {
            // the kernel's own begin/end timestamps (hipExtLaunchKernel events), on its launch stream
            hipEvent_t a = c->take_event(), b = c->take_event();
            // ... and of the repair launch behind a tightened row (timer "trace_repair": the trace figure does not contain it)
            const bool rep = pass > 0 && pass < kMaxPasses && Q.tight_groups[pass];
            hipEvent_t ra = rep ? c->take_event() : nullptr, rb = rep ? c->take_event() : nullptr;
            bool launched = false;
            launch_trace(Q, pass, &pa, c->stats_mode, s, a, b, ra, rb, &launched);
            c->timers[pass == 0 ? "trace0" : "trace"].pending.emplace_back(a, b);
            if (launched) c->timers["trace_repair"].pending.emplace_back(ra, rb);
            else if (rep) { c->event_pool.push_back(ra); c->event_pool.push_back(rb); }
        } else {
            launch_trace(Q, pass, &pa, c->stats_mode, s);
        }
        if (c->roctx) roctx_pop();
        { KernelEvents t(c, "shade"); launch_shade(Q, pass, s, t.a, t.b); }
        if (Q.prov) { KernelEvents t(c, "gather"); launch_echo_gather(Q, pass, s, t.a, t.b); }
        if (wo) { KernelEvents t(c, "waves"); launch_wave_gather(Q, pass, *wo, s, t.a, t.b); }
        if (da) { KernelEvents t(c, "rates"); launch_rate_gather(Q, pass, *da, s, t.a, t.b); }
        if (pass < g.n_reflections - 1) { KernelEvents t(c, "scan"); launch_scan(Q, pass, s, t.a, t.b); }
    }
    { KernelEvents t(c, "column"); launch_column(Q, s, t.a, t.b); }
    if (Q.label_cols) {
        KernelEvents t(c, "label");
        const bool den = Q.signal_denoising > 0;
        launch_label(Q.prov, Q.prov_count, (size_t)Q.prov_cap, Q.n_seg, Q.n_cells, den ? Q.smear_w : 1, den ? Q.smear_mode : 0, den ? Q.smear : nullptr,
                     Q.label_cols, Q.face_cols, s, t.a, t.b);
    }
    if (da) {       // Doppler: the lane's echo lists -> the shifted list, which the column step replays as a list-only stream (rr_debug_column's form)
        { KernelEvents t(c, "shift"); launch_doppler_shift(Q, *da, s, t.a, t.b); }
        { KernelEvents t(c, "column"); launch_column(*side.Qlist, s, t.a, t.b); }
        if (da->vel_cols) { KernelEvents t(c, "winner"); launch_vel_winner(Q, *da, s, t.a, t.b); }
    }
    return 0;
}

// the lane's record of this chain's shape: found, or made new in place of the least recently used of 12
Lane::FrameGraph* find_graph(Lane& L, int az_begin, int az_end, int n_frames, const uint8_t* d_cols_u8, const Params& P)
{
    Lane::FrameGraph* fg = nullptr;
    for (Lane::FrameGraph& x : L.graphs)
        if (x.az_begin == az_begin && x.az_end == az_end && x.n_frames == n_frames && x.cols == (const void*)d_cols_u8 &&
            std::memcmp(x.rows, P.tight_groups, sizeof(x.rows)) == 0) { fg = &x; break; }
    if (!fg) {
        if (L.graphs.size() >= 12) {           // forget the least recently used shape
            size_t lru = 0;
            for (size_t k = 1; k < L.graphs.size(); k++) if (L.graphs[k].last_use < L.graphs[lru].last_use) lru = k;
            drop_graph(L.graphs[lru]);
            L.graphs.erase(L.graphs.begin() + (long)lru);
        }
        Lane::FrameGraph n;
        n.az_begin = az_begin; n.az_end = az_end; n.n_frames = n_frames; n.cols = d_cols_u8;
        std::memcpy(n.rows, P.tight_groups, sizeof(n.rows));
        L.graphs.push_back(n);
        fg = &L.graphs.back();
    }
    return fg;
}

// the second call with a shape: the chain is captured and instantiated (fg->ge set), or the shape stays with plain launches
void capture_graph(rr_ctx* c, Lane::FrameGraph* fg, const Params& P, const PoseArgs& pa, const rr_config& g, hipStream_t s)
{
    // (No SDMA worker may be waiting on an event of this stream while it captures: the runtime treats a
    // hipEventSynchronize on an event whose stream is capturing as an error and invalidates the capture -- found by
    // fuzz_batch in round 6.  Captures are rare, once per shape: let the deliveries in flight finish first.)
    if (c->sdma) sdma_wait_all(c->sdma);
    hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        const int rcq = issue_chain(c, P, pa, g, s);
        hipGraph_t gph = nullptr;
        e = hipStreamEndCapture(s, &gph);
        if (rcq == 0 && e == hipSuccess && gph) {
            hipGraphExec_t ge = nullptr, ge2 = nullptr;
            if (hipGraphInstantiate(&ge, gph, nullptr, nullptr, 0) == hipSuccess && hipGraphInstantiate(&ge2, gph, nullptr, nullptr, 0) == hipSuccess &&
                hipEventCreateWithFlags(&fg->ev[0], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&fg->ev[1], hipEventDisableTiming) == hipSuccess) {
                size_t nn = 0; (void)hipGraphGetNodes(gph, nullptr, &nn);
                std::vector<hipGraphNode_t> nodes(nn); (void)hipGraphGetNodes(gph, nodes.data(), &nn);
                for (hipGraphNode_t nd : nodes) {
                    hipGraphNodeType ty; hipKernelNodeParams kp{};
                    if (hipGraphNodeGetType(nd, &ty) == hipSuccess && ty == hipGraphNodeTypeKernel &&
                        hipGraphKernelNodeGetParams(nd, &kp) == hipSuccess && kp.func == trace0_kernel(P.spill_depth > 0, P.stackless != 0)) {
                        fg->pose_node = nd; fg->pose_kp = kp; fg->pose_P = P; break;
                    }
                }
                if (fg->pose_node) { fg->g = gph; fg->ge = ge; fg->ge2 = ge2; c->graph_captures++; }
                else { (void)hipGraphExecDestroy(ge); (void)hipGraphExecDestroy(ge2); (void)hipGraphDestroy(gph); }
            } else { if (ge) (void)hipGraphExecDestroy(ge); if (ge2) (void)hipGraphExecDestroy(ge2); (void)hipGraphDestroy(gph); }
            if (!fg->ge) for (int k = 0; k < 2; k++) if (fg->ev[k]) { (void)hipEventDestroy(fg->ev[k]); fg->ev[k] = nullptr; }
        } else if (gph) (void)hipGraphDestroy(gph);
    }
    (void)hipGetLastError();
    if (!fg->ge) fg->hits = -1000000;      // capture is not available here: stay with plain launches for this shape
}

// one hipGraphLaunch with the call's poses, on the exec of this shape whose turn it is
int replay_graph(rr_ctx* c, Lane::FrameGraph* fg, const PoseArgs& pa, hipStream_t s)
{
    int pass0 = 0;
    void* args[3] = { (void*)&fg->pose_P, (void*)&pass0, (void*)&pa };
    hipKernelNodeParams kp = fg->pose_kp;
    kp.kernelParams = args; kp.extra = nullptr;
    hipError_t e = hipSuccess;
    const int w = fg->flip; fg->flip ^= 1;
    hipGraphExec_t ex = w ? fg->ge2 : fg->ge;
    if (fg->ev_pending[w]) { HostProfScope hp(6, "ctx:   graph: wait for the exec's previous launch"); e = hipEventSynchronize(fg->ev[w]); fg->ev_pending[w] = false; }
    { HostProfScope hp(3, "ctx:   graph: set the poses"); if (e == hipSuccess) e = hipGraphExecKernelNodeSetParams(ex, fg->pose_node, &kp); }
    { HostProfScope hp(4, "ctx:   graph: launch"); if (e == hipSuccess) e = hipGraphLaunch(ex, s); }
    if (e == hipSuccess) { e = hipEventRecord(fg->ev[w], s); fg->ev_pending[w] = e == hipSuccess; }
    if (e != hipSuccess) return fail(c, -100, std::string("launch graph replay: ") + hipGetErrorString(e));
    c->graph_replays++;
    return 0;
}

// a pose batch rendered on lane L and assembled into dst (rr_simulate_batch_device, rr_simulate_batch_host_async)
int render_batch(rr_ctx* c, Lane& L, const float* poses, int n_frames, uint8_t* dst, hipStream_t s)
{
    FrameJob job; job.n_frames = n_frames;
    const int rc = run_frame(c, L, poses, 0, c->cfg.n_angles, s, job); if (rc) return rc;
    return assemble_frames(c, L, dst, n_frames, s);
}

// rr_simulate_columns_device (one frame, optional f32 columns) and rr_simulate_batch_columns_device after their checks
int simulate_columns(rr_ctx* c, const float* poses, int n_frames, int az_begin, int az_end, uint8_t* d_cols_u8, float* d_cols_f32,
                     void* stream)
{
    RR_HIP(c, hipSetDevice(c->device));
    // rotate over the frame lanes so that calls issued on DIFFERENT streams (pipelined multi-GPU slots) can overlap; a
    // lane is reused only after its previous frame finished
    hipStream_t s = stream_of(c, stream);
    const size_t li = c->next_lane++ % c->lanes.size();
    Lane& L = c->lanes[li];
    FrameJob job; job.n_frames = n_frames; job.d_cols_u8 = d_cols_u8; job.d_cols_f32 = d_cols_f32;
    int rc;
    { HostProfScope hp(0, "ctx: wait for the lane's event");
      rc = take_lane(c, li, s); if (rc) return rc; }
    { HostProfScope hp(1, "ctx: run_frame");
      rc = run_frame(c, L, poses, az_begin, az_end, s, job); if (rc) return rc; }
    { HostProfScope hp(2, "ctx: record the lane's event");
      RR_HIP(c, give_lane(L, s)); }
    return 0;
}

// rr_assemble_image_device (blocks = false: whole frames) / _blocks_device / _frames_device: checked, one launch on `stream`
int assemble_device(rr_ctx* c, const char* who, bool blocks, const uint8_t* d_cols_u8, int n_loc, size_t block_stride, int n_frames,
                    size_t frame_stride, uint8_t* d_imgs_u8, void* stream)
{
    if (!c) return -1;
    if (!c->have_cfg) return fail(c, -2, "rr_set_config has not been called");
    if (!d_cols_u8 || !d_imgs_u8) return fail(c, -3, std::string(who) + ": null buffer");
    if (blocks && (n_loc < 1 || c->cfg.n_angles % n_loc != 0)) return fail(c, -3, std::string(who) + ": n_loc must divide n_angles");
    if (n_frames < 1 || n_frames > RR_MAX_BATCH) return fail(c, -3, std::string(who) + ": n_frames must be 1..64");
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    { TimedScope t(c, s, "assemble"); launch_assemble_u8(d_cols_u8, d_imgs_u8, c->cfg.n_angles, c->cfg.n_cells, c->cfg.scroll_image, s, n_loc, block_stride, n_frames, frame_stride); }
    RR_HIP(c, hipGetLastError());
    return 0;
}

}  // namespace

void drop_graphs(Lane& L)
{
    for (Lane::FrameGraph& fg : L.graphs) drop_graph(fg);
    L.graphs.clear();
}

// The lane's provenance buffers for its current frame buffers (after prepare_lane).  A segment's list holds at most the lane's signal
// capacity (every pass' wave bound, twice that with record_multi_path) -- the list k_column reads -- plus the last pass' slot bound
int ensure_prov_buffers(rr_ctx* c, Lane& L)
{
    const rr_config g = eff_config(c);
    const int n_beam = (int)(c->beams.size() / 3);
    const int last = std::max(0, g.n_reflections - 1);
    const long last_bound = std::min<long>((long)L.buf_cap, last < 20 ? (long)n_beam << last : (long)L.buf_cap);
    const int echo_cap = L.buf_sigcap + (int)last_bound * (g.record_multi_path ? 2 : 1);
    if (L.d_prov.p && L.prov_seg >= L.buf_seg && L.prov_cap == echo_cap && L.prov_cells == L.buf_cells) return 0;
    const size_t S = (size_t)L.buf_seg;
    size_t free_b = 0, total_b = 0;
    RR_HIP(c, hipMemGetInfo(&free_b, &total_b));
    if (S * ((size_t)echo_cap * sizeof(EchoSrc) + (size_t)L.buf_cells * 8) > total_b / 2)
        return fail(c, -6, "the echo lists of a provenance call need more than half of device memory; fewer frames per call or a lower max_waves_per_azimuth");
    RR_HIP(c, hipDeviceSynchronize());      // a provenance chain in flight may still use the old buffers
    RR_HIP(c, L.d_prov.ensure(S * (size_t)echo_cap));
    RR_HIP(c, L.d_prov_count.ensure(S));
    RR_HIP(c, L.d_label_cols.ensure(S * (size_t)L.buf_cells));
    RR_HIP(c, L.d_face_cols.ensure(S * (size_t)L.buf_cells));
    L.prov_seg = L.buf_seg; L.prov_cap = echo_cap; L.prov_cells = L.buf_cells;
    return 0;
}

// Size the lane's frame buffers for n_seg segments under the CURRENT config.  This is the one place
// that decides whether the buffers fit (segments, wave / signal capacity, n_cells, traversal stack):
// every entry point sizes through here BEFORE it takes a pointer into the lane, and run_frame()
// resolves "the lane's own column buffer" only after it -- a reallocation can never leave a caller
// with a stale pointer.  Frames still in flight may use the old buffers: drain the device first.
int prepare_lane(rr_ctx* c, Lane& L, int n_seg, bool want_f32)
{
    const rr_config g = eff_config(c);      // (a parameter batch may ask for more passes than the config)
    const int n_beam = (int)(c->beams.size() / 3);
    const int cap = wave_capacity(g, n_beam);
    const int sigcap = signal_capacity(g, n_beam, cap);
    // a parameter batch (its sets bring their own numbers of passes, so the nominal capacity changes from call to call)
    // also runs in buffers that are LARGER than it needs: the kernels take every stride from the lane (Params::cap), and
    // with the default capacity nothing can overflow that would not have overflowed the nominal one.  Ordinary frames keep
    // the exact layout (a user-lowered max_waves_per_azimuth must be reported when exceeded).
    const bool roomy = c->passes_override >= 0 && c->cfg.max_waves_per_azimuth <= 0 && L.buf_cap >= cap && L.buf_sigcap >= sigcap &&
                       L.buf_passes >= g.n_reflections;
    const bool fits = L.buf_seg >= n_seg && g.n_cells == L.buf_cells &&
                      ((cap == L.buf_cap && sigcap == L.buf_sigcap && L.buf_passes >= g.n_reflections) || roomy) &&
                      (!want_f32 || (L.d_cols_f32.p && L.d_cols_f32.n >= (size_t)L.buf_seg * g.n_cells));
    if (fits) return 0;
    RR_HIP(c, hipDeviceSynchronize());
    return ensure_frame_buffers(c, L, std::max(n_seg, L.buf_seg), want_f32);
}

bool host_visible(const void* p)
{
    hipPointerAttribute_t at;
    const bool v = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();     // a pageable pointer makes hipPointerGetAttributes fail: not an error of the caller's call
    return v;
}

// the lane's deliveries (slot `slot`, or both; only those to `only_dst` if given) have left its image buffers -- over long
// before a lane comes round again
int settle_lane(rr_ctx* c, Lane& L, int slot, const void* only_dst)
{
    for (int b = 0; b < 2; b++) {
        if ((slot >= 0 && b != slot) || (only_dst && L.slot[b].dst != only_dst)) continue;
        const int rc = wait_delivery(c, L.slot[b]); if (rc) return rc;
    }
    return 0;
}

// A frame entry point takes lane li once its arguments have passed: the lane's delivery slots are settled (both, or only
// the one rr_simulate_batch_host_async is about to reuse), rr_get_stats & co. read it from now on, and `s` waits for the
// lane's previous user (its frame buffers) -- no stream: no wait (rr_simulate_device while the caller captures)
int take_lane(rr_ctx* c, size_t li, hipStream_t s, int slot)
{
    Lane& L = c->lanes[li];
    const int rc = settle_lane(c, L, slot); if (rc) return rc;
    c->last_lane = li;
    if (s && L.pending_consume) RR_HIP(c, hipStreamWaitEvent(s, L.ev_consumed, 0));
    return 0;
}

// ... and hands it back: the lane's next user waits for what `s` holds so far
hipError_t give_lane(Lane& L, hipStream_t s)
{
    const hipError_t e = hipEventRecord(L.ev_consumed, s);
    L.pending_consume = true;
    return e;
}

int run_frame(rr_ctx* c, Lane& L, const float* pose, int az_begin, int az_end, hipStream_t s, const FrameJob& job)
{
    const int n_frames = job.n_frames, provenance = job.provenance;
    const float4* d_matsets = job.d_matsets; const WaveOut* paths = job.paths; const DopArgs* doppler = job.doppler;
    const rr_config g = eff_config(c);      // (a parameter batch may ask for more passes than the config)
    if (az_begin < 0 || az_end > g.n_angles || az_begin > az_end) return fail(c, -3, "azimuth range out of bounds");
    const int n_loc = az_end - az_begin;
    const int n_seg = n_loc * n_frames;
    if (n_seg == 0) return 0;
    if (n_frames < 1 || n_frames > RR_MAX_BATCH) return fail(c, -3, "frame batch must be 1..64");
    for (int k = 0; k < 7 * (d_matsets ? 1 : n_frames); k++) if (!std::isfinite(pose[k])) return fail(c, -3, "non-finite pose");
    int rc = upload_tables(c); if (rc) return rc;
    // ONE per-azimuth pose table and several frames: every frame would be the same sweep and the call's poses would be ignored
    // without a word (advisor, round 5) -- a batch under include_motion brings one table per frame (or k tables, frame f -> f % k)
    if (!d_matsets && n_frames > 1 && !c->motion.empty() && c->motion_rows == 1)
        return fail(c, -3, "a pose batch while ONE per-azimuth pose table is set (rr_set_motion_poses): give one table per frame (k x n_angles poses) or clear the table");
    if (provenance && d_matsets) return fail(c, -3, "echo provenance is for pose batches: the frames of a parameter batch share the hits of pass 0");
    if (paths && d_matsets) return fail(c, -3, "wave paths are for pose batches: the frames of a parameter batch share the hits of pass 0");
    if (doppler && (d_matsets || !provenance)) return fail(c, -3, "Doppler is for pose batches with their echo lists: the frames of a parameter batch share the hits of pass 0");
    rc = prepare_lane(c, L, n_seg, job.lane_f32); if (rc) return rc;
    if (provenance) { rc = ensure_prov_buffers(c, L); if (rc) return rc; }
    DopArgs da{};
    if (doppler) {
        rc = ensure_dop_buffers(c, L, doppler->vel_cols != nullptr); if (rc) return rc;
        da = *doppler;
        da.in = L.d_dop_in.p; da.n_objects = c->n_objects; da.wstate = L.d_dop_state.p; da.rate = L.d_dop_rate.p; da.count = L.d_dop_count.p;
        da.shifted = L.d_dop_sig.p; da.vel_cols = doppler->vel_cols ? L.d_dop_vel_cols.p : nullptr;
        // the sensor's velocities and the twists ride down behind the lane's previous user.  The host array lives with the lane; the
        // copy of the lane's previous Doppler call has left it before it is written again
        if (L.pending_consume) RR_HIP(c, hipEventSynchronize(L.ev_consumed));
        L.h_dop_in.assign(64 + 2 * (size_t)c->n_objects, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        const float* v = job.sensor_vel;
        for (int f = 0; f < n_frames && v; f++) L.h_dop_in[(size_t)f] = make_float4(v[3 * f], v[3 * f + 1], v[3 * f + 2], 0.0f);
        for (size_t o = 0; o < (size_t)c->n_objects && 6 * o + 5 < c->twists.size(); o++) {
            const float* t = c->twists.data() + 6 * o;
            L.h_dop_in[64 + 2 * o] = make_float4(t[0], t[1], t[2], 0.0f); L.h_dop_in[64 + 2 * o + 1] = make_float4(t[3], t[4], t[5], 0.0f);
        }
        RR_HIP(c, hipMemcpyAsync(L.d_dop_in.p, L.h_dop_in.data(), L.h_dop_in.size() * sizeof(float4), hipMemcpyHostToDevice, s));
    }
    WaveOut wo{};
    if (paths) { rc = ensure_path_state(c, L); if (rc) return rc; wo = *paths; wo.state = L.d_path_state.p; }
    uint8_t* d_cols_u8 = job.d_cols_u8 ? job.d_cols_u8 : L.d_cols_u8.p;       // the lane's own column buffer, valid only from here on
    float* d_cols_f32 = job.lane_f32 ? L.d_cols_f32.p : job.d_cols_f32;
    Params P;
    fill_params(c, L, P, pose, az_begin, n_seg, d_cols_u8, d_cols_f32);
    P.n_loc = n_loc; P.n_frames = n_frames;
    if (provenance) {
        P.prov = L.d_prov.p; P.prov_count = L.d_prov_count.p; P.prov_cap = L.prov_cap;
        if (provenance > 1) { P.label_cols = L.d_label_cols.p; P.face_cols = L.d_face_cols.p; }
    }
    if (d_matsets) {   // parameter batch: one pose, one material table per frame
        P.materials = d_matsets; P.mat_limits = L.d_matset_limits.p; P.mat_stride = job.mat_stride;
        P.set_mode = 1;
        P.noise_rows = 1;     // every set is the SAME frame under another parameter set: one noise realisation (row 0)
        P.motion_rows = 1;    // ... and one sweep of the antenna (table 0); every set the SAME pose: q_sm / t_sm (no pose table)
        SetPlan dflt;
        const SetPlan* plan = job.plan;
        if (!plan) {          // material sets only: one beam, every frame the config's passes
            for (int f = 0; f < n_frames; f++) { dflt.frame_passes[f] = (unsigned char)g.n_reflections; dflt.frame_beam[f] = 0; }
            dflt.group_frame[0] = 0; plan = &dflt;
        }
        P.n_groups = plan->n_groups;
        std::memcpy(P.frame_passes, plan->frame_passes, (size_t)n_frames);
        std::memcpy(P.frame_beam, plan->frame_beam, (size_t)n_frames);
        std::memcpy(P.group_frame, plan->group_frame, (size_t)plan->n_groups);
        if (plan->d_beams) { P.beams = plan->d_beams; P.beam_order = plan->d_order; P.beam_order2 = plan->d_order2; }
    }
    if (c->stats_mode || g.n_reflections == 0) RR_HIP(c, hipMemsetAsync(L.d_counters.p, 0, sizeof(Counters), s));
    if (provenance && g.n_reflections == 0) RR_HIP(c, hipMemsetAsync(L.d_prov_count.p, 0, (size_t)n_seg * sizeof(uint32_t), s));     // no pass, no gather launch
    if (doppler && g.n_reflections == 0) RR_HIP(c, hipMemsetAsync(da.count, 0, (size_t)n_seg * sizeof(uint32_t), s));     // no pass, no gather launch
    if (paths && g.n_reflections == 0) {      // no pass, no gather launch
        if (wo.counts) RR_HIP(c, hipMemsetAsync(wo.counts, 0, (size_t)n_seg * sizeof(uint32_t), s));
        if (wo.pass_counts) RR_HIP(c, hipMemsetAsync(wo.pass_counts, 0, (size_t)n_seg * kWavePasses * sizeof(uint32_t), s));
    }
    L.last_n_seg = n_seg; L.last_n_passes = g.n_reflections;
    rc = choose_trace_rows(c, L, P, g, s); if (rc) return rc;
    // the poses of the call ride in the pass-0 trace launch (by value), which also writes them into the lane's pose table for
    // the launches behind it; a parameter batch (every set the same pose) and a single frame use row 0
    PoseArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.n = d_matsets ? 1 : n_frames;
    for (int f = 0; f < pa.n; f++) for (int k = 0; k < 7; k++) pa.p[f][k] = pose[7 * f + k];
    P.pose_table = reinterpret_cast<float4*>(L.d_poses.p);
    // Launch graphs: a chain that has been issued before with the same shape is captured once and replayed -- one
    // hipGraphLaunch instead of 4..20 launches (host time per device entry of rr_multi: 45-81 -> ~25 us).  Only plain pose
    // batches: no parameter batch, no timing / statistics / roctx instrumentation, no provenance or paths chain (which
    // does not even look at the lane's graphs: a plain batch afterwards replays as before); whatever a captured launch bakes in is
    // covered by graph_gen (tables, tree, lane buffers) or by the key (azimuth block, frames, output buffer, trace rows)
    if (L.graph_gen != c->graph_gen) { drop_graphs(L); L.graph_gen = c->graph_gen; }
    const bool graphable = !(provenance || paths || doppler) && !d_matsets && !d_cols_f32 && c->use_graphs && !c->timing && !c->stats_mode && !c->roctx && g.n_reflections > 0;
    if (graphable) {
        Lane::FrameGraph* fg = find_graph(L, az_begin, az_end, n_frames, d_cols_u8, P);
        fg->last_use = ++c->graph_clock;
        if (!fg->ge && fg->hits >= 1) capture_graph(c, fg, P, pa, g, s);        // the second call with this shape: worth a capture
        if (fg->ge) return replay_graph(c, fg, pa, s);
        fg->hits++;
    }
    Params Plist;
    ChainSide side; side.wo = paths ? &wo : nullptr;
    if (doppler) {      // the list-only form of the column launch: two passes on paper, the list = the shifted echoes, no slot of a last pass
        side.da = &da; side.Qlist = &Plist;
        Plist = P;
        Plist.n_passes = 2; Plist.sig = da.shifted; Plist.sig_count = da.count; Plist.sigcap = L.prov_cap;
        Plist.count[1] = L.d_dop_zero.p; Plist.seg_stats = L.d_dop_stats.p;      // (the chain's own statistics stay as its k_column left them)
        Plist.hist_host = nullptr; Plist.grid_hint = nullptr;
    }
    { HostProfScope hp(5, "ctx:   chain issued kernel by kernel");
      const int rcq = issue_chain(c, P, pa, g, s, side); if (rcq) return rcq; }
    RR_HIP(c, hipGetLastError());
    return 0;
}

// the lane's columns of n_frames whole frames -> images [n_frames][n_cells][n_angles] in dst, on s
int assemble_frames(rr_ctx* c, const Lane& L, uint8_t* dst, int n_frames, hipStream_t s)
{
    const rr_config& g = c->cfg;
    const size_t npx = (size_t)g.n_angles * g.n_cells;
    { TimedScope t(c, s, "assemble");
      launch_assemble_u8(L.d_cols_u8.p, dst, g.n_angles, g.n_cells, g.scroll_image, s, g.n_angles, npx, n_frames, npx); }
    RR_HIP(c, hipGetLastError());
    return 0;
}

}  // namespace rr

extern "C" {

int rr_simulate_columns_device(rr_ctx* c, const float pose[7], int az_begin, int az_end,
                               uint8_t* d_cols_u8, float* d_cols_f32, void* stream)
{
    int rc = check_ready(c); if (rc) return rc;
    if (!pose || !d_cols_u8) return fail(c, -3, "rr_simulate_columns_device: null pose/output");
    return simulate_columns(c, pose, 1, az_begin, az_end, d_cols_u8, d_cols_f32, stream);
}

int rr_simulate_batch_columns_device(rr_ctx* c, const float* poses, int n_frames, int az_begin, int az_end,
                                     uint8_t* d_cols_u8, void* stream)
{
    int rc = check_ready(c); if (rc) return rc;
    if (!poses || !d_cols_u8) return fail(c, -3, "rr_simulate_batch_columns_device: null poses/output");
    return simulate_columns(c, poses, n_frames, az_begin, az_end, d_cols_u8, nullptr, stream);
}

int rr_simulate_batch_device(rr_ctx* c, const float* poses, int n_frames, uint8_t* d_imgs_u8, void* stream)
{
    int rc = check_ready(c); if (rc) return rc;
    if (!poses || !d_imgs_u8) return fail(c, -3, "rr_simulate_batch_device: null poses/output");
    if (n_frames < 1 || n_frames > RR_MAX_BATCH) return fail(c, -3, "rr_simulate_batch_device: n_frames must be 1..64");
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    rc = upload_tables(c); if (rc) return rc;
    const size_t li = c->next_lane++ % c->lanes.size();
    Lane& L = c->lanes[li];
    rc = take_lane(c, li, s); if (rc) return rc;
    rc = render_batch(c, L, poses, n_frames, d_imgs_u8, s); if (rc) return rc;
    RR_HIP(c, give_lane(L, s));
    return 0;
}

int rr_deliver_to_host_async(rr_ctx* c, const void* d_src, void* h_dst, size_t bytes, void* stream)
{
    if (!c) return -1;
    if (bytes == 0) return 0;
    if (!d_src || !h_dst) return fail(c, -3, "rr_deliver_to_host_async: null pointer");
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    hipEvent_t ev = nullptr;
    if (!c->delivery_events.empty()) { ev = c->delivery_events.back(); c->delivery_events.pop_back(); }
    else RR_HIP(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    const bool visible = host_visible(h_dst);
    SdmaCopier* sd = visible ? sdma_of(c, d_src) : nullptr;
    uint64_t job = 0;
    if (sd) {
        const hipError_t e = hipEventRecord(ev, s);        // the copy starts once the stream has got here
        if (e != hipSuccess) { c->delivery_events.push_back(ev); RR_HIP(c, e); }
        job = sdma_submit(sd, ev, d_src, h_dst, bytes);
    } else {
        const int rc = copy_out(c, d_src, h_dst, bytes, visible, s);
        if (rc) { c->delivery_events.push_back(ev); return rc; }
        const hipError_t e = hipEventRecord(ev, s);        // ... is complete once the stream has got here
        if (e != hipSuccess) { c->delivery_events.push_back(ev); RR_HIP(c, e); }
    }
    Delivery d; d.ev = ev; d.dst = h_dst; d.job = job;
    c->deliveries.push_back(std::move(d));
    return 0;
}

int rr_host_delivery_route(rr_ctx* c)
{
    if (!c) return -1;
    if (c->sdma && c->host_sdma && !sdma_failed(c->sdma, nullptr)) return 2;      // SDMA through ROCr: in use
    if (c->host_sdma && !c->sdma_tried) return 1;                                  // ... will be tried by the first delivery
    return 0;                                                                      // stream-ordered copies behind the batch (copy_out)
}

int rr_copy_to_host_async(rr_ctx* c, const void* d_src, void* h_dst, size_t bytes, void* stream)
{
    if (!c) return -1;
    if (bytes && (!d_src || !h_dst)) return fail(c, -3, "rr_copy_to_host_async: null pointer");
    RR_HIP(c, hipSetDevice(c->device));
    return copy_out(c, d_src, h_dst, bytes, bytes > 0 && host_visible(h_dst), stream_of(c, stream));
}

int rr_simulate_batch_host_async(rr_ctx* c, const float* poses, int n_frames, uint8_t* h_imgs_u8, void* stream)
{
    int rc = check_ready(c); if (rc) return rc;
    if (!poses || !h_imgs_u8) return fail(c, -3, "rr_simulate_batch_host_async: null poses/output");
    if (n_frames < 1 || n_frames > RR_MAX_BATCH) return fail(c, -3, "rr_simulate_batch_host_async: n_frames must be 1..64");
    RR_HIP(c, hipSetDevice(c->device));
    const rr_config& g = c->cfg;
    hipStream_t s = stream_of(c, stream);
    rc = upload_tables(c); if (rc) return rc;
    const size_t li = c->next_lane++ % c->lanes.size();
    Lane& L = c->lanes[li];
    const size_t bytes = (size_t)n_frames * g.n_cells * g.n_angles;
    // The default route: over the SDMA engines through ROCr, at once, behind this batch's assemble -- no shader core stores a
    // byte of it, so the batches beside it run at their HBM-resident rate, and it is the same engine under every HIP runtime.
    // The fallback (SDMA switched off or not available, a pageable destination, statistics mode): the images leave on a plain
    // copy behind the batch, on its stream (copy_out).  Stores to host memory drain at PCIe speed, and the stores of the
    // kernels beside them wait behind them: on the target this route delivers some 7 % fewer images/s than SDMA
    const bool device_visible = host_visible(h_imgs_u8);
    SdmaCopier* sd = (device_visible && !c->stats_mode) ? sdma_of(c, c->d_bvh.p) : nullptr;
    const int b = L.next_slot;
    Delivery& d = L.slot[b];
    rc = take_lane(c, li, s, b); if (rc) return rc;         // the copy that empties THIS buffer: two uses of the lane ago
    if (d.img.n < bytes) {
        rc = settle_lane(c, L); if (rc) return rc;
        RR_HIP(c, hipDeviceSynchronize());                  // an earlier batch may still use the old buffer
        RR_HIP(c, d.img.ensure(bytes));
    }
    rc = render_batch(c, L, poses, n_frames, d.img.p, s); if (rc) return rc;
    if (sd) {
        RR_HIP(c, hipEventRecord(d.ev, s));
        d.job = sdma_submit(sd, d.ev, d.img.p, h_imgs_u8, bytes);
    } else {
        rc = copy_out(c, d.img.p, h_imgs_u8, bytes, device_visible, s); if (rc) return rc;
        RR_HIP(c, hipEventRecord(d.ev, s));
    }
    d.dst = h_imgs_u8;
    L.next_slot ^= 1;
    RR_HIP(c, give_lane(L, s));       // what the lane's next user waits for: the batch and its copy
    return 0;
}

int rr_wait_host(rr_ctx* c, const void* h_imgs_u8)
{
    if (!c) return -1;
    RR_HIP(c, hipSetDevice(c->device));
    // oldest batch first (lanes are handed out round robin: the next one to be used holds the oldest batch): its images leave
    // while the younger batches still render, and only the youngest batch's copy is left when the kernels are done -- in lane
    // order the youngest batch may come first, and the copies of all the others then queue up behind the end of the run
    for (size_t i = 0; i < c->deliveries.size();) {       // rr_deliver_to_host_async's copies
        Delivery& d = c->deliveries[i];
        if (h_imgs_u8 != nullptr && d.dst != h_imgs_u8) { i++; continue; }
        const int rc = wait_delivery(c, d); if (rc) return rc;
        c->delivery_events.push_back(d.ev);
        c->deliveries.erase(c->deliveries.begin() + (long)i);
    }
    const size_t nl = c->lanes.size();
    for (size_t k = 0; k < nl; k++) { const int rc = settle_lane(c, c->lanes[(c->next_lane + k) % nl], -1, h_imgs_u8); if (rc) return rc; }
    return 0;
}

int rr_assemble_image_device(rr_ctx* c, const uint8_t* d_cols_u8, uint8_t* d_img_u8, void* stream)
{
    return assemble_device(c, "rr_assemble_image_device", false, d_cols_u8, 0, 0, 1, 0, d_img_u8, stream);
}

int rr_assemble_frames_device(rr_ctx* c, const uint8_t* d_cols_u8, int n_loc, size_t block_stride,
                              int n_frames, size_t frame_stride, uint8_t* d_imgs_u8, void* stream)
{
    return assemble_device(c, "rr_assemble_frames_device", true, d_cols_u8, n_loc, block_stride, n_frames, frame_stride, d_imgs_u8, stream);
}

int rr_assemble_blocks_device(rr_ctx* c, const uint8_t* d_cols_u8, int n_loc, size_t block_stride,
                              uint8_t* d_img_u8, void* stream)
{
    return assemble_device(c, "rr_assemble_blocks_device", true, d_cols_u8, n_loc, block_stride, 1, 0, d_img_u8, stream);
}

int rr_simulate_device(rr_ctx* c, const float pose[7], uint8_t* d_img_u8, void* stream)
{
    int rc = check_ready(c); if (rc) return rc;
    if (!pose || !d_img_u8) return fail(c, -3, "rr_simulate_device: null pose/output");
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t user = stream_of(c, stream);
    rc = upload_tables(c); if (rc) return rc;
    const int A = c->cfg.n_angles;
    if (c->lanes.size() == 1) {
        Lane& L = c->lanes[0];
        // With ONE lane every launch of the frame goes to the caller's stream, so the call can be CAPTURED into a hipGraph
        // (hipStreamBeginCapture on `user`, this call, hipStreamEndCapture) and replayed -- tools/cpp_bench.cpp `graph`.  While
        // capturing, the lane's hand-over event stays out of it (an event recorded outside the capture cannot be waited
        // for inside): the caller keeps other work off the context while such a graph runs.
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(user, &cap);
        const bool capturing = cap == hipStreamCaptureStatusActive;
        // the lane's previous frame may have run on ANOTHER caller stream (or a flushed host copy may still read the lane)
        rc = take_lane(c, 0, capturing ? nullptr : user); if (rc) return rc;
        rc = run_frame(c, L, pose, 0, A, user); if (rc) return rc;
        rc = rr_assemble_image_device(c, L.d_cols_u8.p, d_img_u8, user); if (rc) return rc;
        if (!capturing) RR_HIP(c, give_lane(L, user));
        return 0;
    }
    // Frame pipelining: trace/shade/scan/column of this frame run on the lane's own stream
    // (no dependency on the caller's stream), only the assemble -- the one kernel that touches
    // the caller's buffer -- is ordered on the caller's stream.  The lane is reused only after
    // that assemble has consumed its columns.
    const size_t li = c->next_stream_lane++ % (size_t)c->stream_lanes;
    Lane& L = c->lanes[li];
    rc = take_lane(c, li, L.stream); if (rc) return rc;
    rc = run_frame(c, L, pose, 0, A, L.stream); if (rc) return rc;
    RR_HIP(c, hipEventRecord(L.ev_ready, L.stream));
    RR_HIP(c, hipStreamWaitEvent(user, L.ev_ready, 0));
    rc = rr_assemble_image_device(c, L.d_cols_u8.p, d_img_u8, user); if (rc) return rc;
    RR_HIP(c, give_lane(L, user));
    return 0;
}

int rr_simulate(rr_ctx* c, const float pose[7], int az_begin, int az_end,
                uint8_t* out_u8, float* out_f32, rr_stats* stats)
{
    int rc = check_ready(c); if (rc) return rc;
    if (!pose || (!out_u8 && !out_f32)) return fail(c, -3, "rr_simulate: null pose/output");
    RR_HIP(c, hipSetDevice(c->device));
    const rr_config& g = c->cfg;
    if (az_begin < 0 || az_end > g.n_angles || az_begin > az_end) return fail(c, -3, "azimuth range out of bounds");
    const int n_seg = az_end - az_begin;
    if (n_seg == 0) { if (stats) std::memset(stats, 0, sizeof(*stats)); return 0; }
    rc = upload_tables(c); if (rc) return rc;
    Lane& L = c->lanes[0];
    // The reference's call shape: one synchronous simulate() per frame (radar_simulator.cpp:197-212).  Its latency is
    // the chain of kernels plus what the host adds around it, so the host adds as little as it can: the frame is
    // ordered behind the lane's previous user by an event (no device-wide drain), the error bits and the per-pass
    // counters ride home behind the image on the same stream, and ONE hipStreamSynchronize ends the call.
    rc = take_lane(c, 0, c->stream); if (rc) return rc;
    FrameJob job; job.lane_f32 = out_f32 != nullptr;
    rc = run_frame(c, L, pose, az_begin, az_end, c->stream, job); if (rc) return rc;
    const size_t n_st = (size_t)n_seg * (size_t)std::max(1, g.n_reflections);
    const size_t need = sizeof(Counters) + (stats ? n_st * sizeof(SegStats) : 0);
    if (c->h_frame_bytes < need) {
        if (c->h_frame) (void)hipHostFree(c->h_frame);
        c->h_frame = nullptr; c->h_frame_bytes = 0;
        RR_HIP(c, hipHostMalloc(&c->h_frame, need + 4096, hipHostMallocDefault));
        c->h_frame_bytes = need + 4096;
    }
    Counters* h_cnt = reinterpret_cast<Counters*>(c->h_frame);
    SegStats* h_ss = reinterpret_cast<SegStats*>(h_cnt + 1);
    std::vector<uint8_t> h8; std::vector<float> hf;
    if (n_seg == g.n_angles) {
        // whole frame: transpose on the GPU, one D2H copy straight into the caller's row-major buffer
        const size_t npx = (size_t)g.n_cells * g.n_angles;
        if (out_u8) {
            DevBuf<uint8_t>& img = L.slot[0].img;      // (settled by take_lane)
            RR_HIP(c, img.ensure(npx));
            launch_assemble_u8(L.d_cols_u8.p, img.p, g.n_angles, g.n_cells, g.scroll_image, c->stream);
            RR_HIP(c, hipMemcpyAsync(out_u8, img.p, npx, hipMemcpyDeviceToHost, c->stream));
        }
        if (out_f32) {
            RR_HIP(c, L.d_img_f32.ensure(npx));
            launch_assemble_f32(L.d_cols_f32.p, L.d_img_f32.p, g.n_angles, g.n_cells, g.scroll_image, c->stream);
            RR_HIP(c, hipMemcpyAsync(out_f32, L.d_img_f32.p, npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        }
    } else {
        h8.resize((size_t)n_seg * g.n_cells);
        hf.resize(out_f32 ? (size_t)n_seg * g.n_cells : 0);
        RR_HIP(c, hipMemcpyAsync(h8.data(), L.d_cols_u8.p, h8.size(), hipMemcpyDeviceToHost, c->stream));
        if (out_f32) RR_HIP(c, hipMemcpyAsync(hf.data(), L.d_cols_f32.p, hf.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    // error bits / counters and the per-pass statistics ride home behind the image.  (Round 6 tried ONE kernel storing both into
    // the page-locked block instead -- k_frame_report, no copy engine involved: 0.151 instead of 0.139-0.141 ms per call on
    // config 2.  This is the latency path; the small copies stay.)
    RR_HIP(c, hipMemcpyAsync(h_cnt, L.d_counters.p, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    if (stats && L.d_seg_stats.p && g.n_reflections > 0)
        RR_HIP(c, hipMemcpyAsync(h_ss, L.d_seg_stats.p, n_st * sizeof(SegStats), hipMemcpyDeviceToHost, c->stream));
    RR_HIP(c, give_lane(L, c->stream));
    RR_HIP(c, hipStreamSynchronize(c->stream));
    if (n_seg != g.n_angles) {
        for (int s = 0; s < n_seg; s++) {
            const int col = (g.scroll_image + az_begin + s) % g.n_angles;   // RadarCPU.cpp:457
            for (int i = 0; i < g.n_cells; i++) {
                if (out_u8) out_u8[(size_t)i * g.n_angles + col] = h8[(size_t)s * g.n_cells + i];
                if (out_f32) out_f32[(size_t)i * g.n_angles + col] = hf[(size_t)s * g.n_cells + i];
            }
        }
    }
    const uint32_t overflow = h_cnt->overflow;
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->nodes_visited = h_cnt->nodes; stats->tris_tested = h_cnt->tris; stats->overflow = overflow;
        if (g.n_reflections > 0)
            for (size_t k = 0; k < n_st; k++) { stats->wave_passes += h_ss[k].wave_passes; stats->hits += h_ss[k].hits; stats->signals += h_ss[k].signals; }
        if (getenv("RR_TRACE_STATS")) { rr_stats tmp; (void)rr_get_stats(c, &tmp); }     // prints the wave-level loop shape
    }
    if (overflow) RR_HIP(c, hipMemset(L.d_sticky.p, 0, sizeof(uint32_t)));   // reported here, not again by rr_synchronize
    return overflow_error(c, overflow);
}

}  // extern "C"
