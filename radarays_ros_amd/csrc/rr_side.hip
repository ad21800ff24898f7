// rr_side.hip -- the entry points of the chains that ride beside the frame chain (run_frame with a FrameJob that asks for them): echo
// provenance, wave paths, Doppler, each as a device form for pose batches and a synchronous host form for one frame, and rr_debug_labels.
// One refusal list (check_side), one batch step (side_batch), one staging step for the host forms (host_lane, a Stage over the lane's pool).
#include "rr_stage.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace rr {
namespace {

// The refusals of the six entry points (nothing is written): what they share, around the feature's own (`own`: the text of its first
// refusal that applies, or null).  rows: a row buffer is given (waves: of wave records, else of echoes); rows_last: what is wrong with
// it is said after everything else, as the host form of the paths call always has
template <class Own>
int check_side(rr_ctx* c, const char* who, const void* poses, int n_frames, const void* imgs, bool waves, bool rows, size_t stride, const void* counts,
               bool rows_last, Own own)
{
    int rc = check_ready(c); if (rc) return rc;
    const std::string w(who);
    const char* no_rows = nullptr;
    if (rows && !counts) no_rows = waves ? ": a wave buffer needs a count buffer" : ": an echo buffer needs a count buffer";
    else if (rows && stride == 0) no_rows = waves ? ": wave_stride must be positive" : ": echo_stride must be positive";
    if (!poses || !imgs) return fail(c, -3, w + ": null poses/output");
    if (n_frames < 1 || n_frames > RR_MAX_BATCH) return fail(c, -3, w + ": n_frames must be 1..64");
    if (no_rows && !rows_last) return fail(c, -3, w + no_rows);
    if (const char* no = own()) return fail(c, -3, w + no);
    if (c->n_objects >= 0xFFFFFFu) return fail(c, -3, w + ": the info word holds object ids below 2^24 - 1");
    if (c->cfg.n_reflections > RR_WAVES_MAX_PASSES) return fail(c, -3, w + ": the info word holds passes below 16 (n_reflections <= 16)");
    if (no_rows) return fail(c, -3, w + no_rows);
    return 0;
}

int check_provenance(rr_ctx* c, const char* who, const void* poses, int n_frames, const void* imgs, const void* echoes, size_t echo_stride,
                     const void* counts)
{
    return check_side(c, who, poses, n_frames, imgs, false, echoes != nullptr, echo_stride, counts, false, [&]() -> const char* {
        return c->cfg.n_cells > kLabelMaxCells ? ": n_cells exceeds RR_LABEL_MAX_CELLS (8192)" : nullptr; });
}

// host_rows: the rows are host memory, filled by memcpy, and need no alignment
int check_paths(rr_ctx* c, const char* who, const void* poses, int n_frames, const void* imgs, const void* waves, size_t wave_stride,
                const void* counts, unsigned flags, bool host_rows)
{
    return check_side(c, who, poses, n_frames, imgs, true, waves != nullptr, wave_stride, counts, host_rows, [&]() -> const char* {
        if (!host_rows && (uintptr_t)waves % 16 != 0) return ": the wave buffer must be 16-byte aligned";
        return (flags & ~(unsigned)RR_WAVES_MAP_FRAME) ? ": unknown flag bits" : nullptr; });
}

int check_doppler(rr_ctx* c, const char* who, const void* poses, int n_frames, const float* sensor_vel, float gain, const void* imgs, const void* vel,
                  const void* cells, size_t echo_stride, const void* counts, const void* vel_img)
{
    return check_side(c, who, poses, n_frames, imgs, false, vel || cells, echo_stride, counts, false, [&]() -> const char* {
        if (!std::isfinite(gain)) return ": non-finite gain";
        for (int k = 0; sensor_vel && k < 3 * n_frames; k++) if (!std::isfinite(sensor_vel[k])) return ": non-finite sensor velocity";
        return vel_img && c->cfg.n_cells > kLabelMaxCells ? ": n_cells exceeds RR_LABEL_MAX_CELLS (8192) with a velocity image" : nullptr; });
}

// A pose batch with a side chain on lane li (taken and handed back here), everything enqueued on s: the chain, the images, and what the
// feature launches behind them (`tail`).  Whole frames: segment = frame * n_angles + azimuth, the layout of the caller's buffers
template <class Tail>
int side_batch(rr_ctx* c, size_t li, const float* poses, const FrameJob& job, uint8_t* d_imgs_u8, hipStream_t s, Tail tail)
{
    Lane& L = c->lanes[li];
    RR_HIP(c, hipSetDevice(c->device));
    int rc = upload_tables(c); if (rc) return rc;
    rc = take_lane(c, li, s); if (rc) return rc;
    rc = run_frame(c, L, poses, 0, c->cfg.n_angles, s, job); if (rc) return rc;
    rc = assemble_frames(c, L, d_imgs_u8, job.n_frames, s); if (rc) return rc;
    tail(L);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, give_lane(L, s));
    return 0;
}

int provenance_batch(rr_ctx* c, size_t li, const float* poses, int n_frames, uint8_t* d_imgs_u8, uint32_t* d_labels, uint32_t* d_faces,
                     rr_echo_src* d_echoes, size_t echo_stride, uint32_t* d_echo_counts, hipStream_t s)
{
    const rr_config& g = c->cfg;
    FrameJob job; job.n_frames = n_frames; job.provenance = (d_labels || d_faces) ? 2 : 1;
    return side_batch(c, li, poses, job, d_imgs_u8, s, [&](Lane& L) {
        { TimedScope t(c, s, "assemble");
          if (d_labels) launch_assemble_u32(L.d_label_cols.p, d_labels, g.n_angles, g.n_cells, g.scroll_image, s, n_frames);
          if (d_faces) launch_assemble_u32(L.d_face_cols.p, d_faces, g.n_angles, g.n_cells, g.scroll_image, s, n_frames); }
        if (d_echo_counts)
            launch_echo_export(L.d_prov.p, L.d_prov_count.p, (size_t)L.prov_cap, n_frames * g.n_angles, d_echoes, d_echoes ? echo_stride : 0, d_echo_counts, s);
    });
}

int paths_batch(rr_ctx* c, size_t li, const float* poses, int n_frames, uint8_t* d_imgs_u8, rr_wave_rec* d_waves, size_t wave_stride,
                uint32_t* d_wave_counts, uint32_t* d_pass_counts, unsigned flags, hipStream_t s)
{
    WaveOut wo;      // (state: the lane's, run_frame)
    wo.recs = reinterpret_cast<float4*>(d_waves); wo.stride = d_waves ? wave_stride : 0;
    wo.counts = d_wave_counts; wo.pass_counts = d_pass_counts; wo.state = nullptr; wo.flags = flags;
    FrameJob job; job.n_frames = n_frames; job.paths = &wo;
    return side_batch(c, li, poses, job, d_imgs_u8, s, [](Lane&) {});
}

// d_img_f32: the f32 image of ONE frame
int doppler_batch(rr_ctx* c, size_t li, const float* poses, int n_frames, const float* sensor_vel, float gain, uint8_t* d_imgs_u8, float* d_img_f32,
                  float* d_echo_vel, size_t echo_stride, uint32_t* d_echo_counts, int32_t* d_echo_cells, float* d_vel_img, hipStream_t s)
{
    const rr_config& g = c->cfg;
    DopArgs da{};      // (the lane's part: run_frame)
    da.gain = gain; da.vel_cols = d_vel_img;      // (non-null: asked for)
    da.echo_vel = d_echo_vel; da.echo_cells = d_echo_cells; da.echo_counts = d_echo_counts; da.stride = (d_echo_vel || d_echo_cells) ? echo_stride : 0;
    FrameJob job; job.n_frames = n_frames; job.lane_f32 = d_img_f32 != nullptr; job.provenance = 1; job.doppler = &da; job.sensor_vel = sensor_vel;
    return side_batch(c, li, poses, job, d_imgs_u8, s, [&](Lane& L) {
        TimedScope t(c, s, "assemble");
        if (d_img_f32) launch_assemble_f32(L.d_cols_f32.p, d_img_f32, g.n_angles, g.n_cells, g.scroll_image, s);
        if (d_vel_img) launch_assemble_u32(reinterpret_cast<const uint32_t*>(L.d_dop_vel_cols.p), reinterpret_cast<uint32_t*>(d_vel_img), g.n_angles, g.n_cells,
                                           g.scroll_image, s, n_frames);
    });
}

// Lane 0 for a host form of one frame: its tables up to date, its deliveries settled (the image is assembled in the buffer of delivery
// slot 0, as rr_simulate does), its frame buffers and that buffer sized
int host_lane(rr_ctx* c, Lane& L, bool want_f32 = false)
{
    RR_HIP(c, hipSetDevice(c->device));
    int rc = upload_tables(c); if (rc) return rc;
    rc = settle_lane(c, L); if (rc) return rc;
    rc = prepare_lane(c, L, c->cfg.n_angles, want_f32); if (rc) return rc;
    RR_HIP(c, L.slot[0].img.ensure((size_t)c->cfg.n_angles * c->cfg.n_cells));
    return 0;
}

// The way out of a host form: its outputs are held (rr_stage.h) -- a call that fails after its chain has run (the frame's error bits
// come home with them) has written nothing.  The lane is handed back behind the copies
int commit_lane(rr_ctx* c, Stage& st, Lane& L) { return st.commit([c] { return report_frame_errors(c); }, &L); }

}  // namespace
}  // namespace rr

extern "C" {

int rr_simulate_batch_provenance_device(rr_ctx* c, const float* poses, int n_frames, uint8_t* d_imgs_u8, uint32_t* d_labels, uint32_t* d_faces,
                                        rr_echo_src* d_echoes, size_t echo_stride, uint32_t* d_echo_counts, void* stream)
{
    int rc = check_provenance(c, "rr_simulate_batch_provenance_device", poses, n_frames, d_imgs_u8, d_echoes, echo_stride, d_echo_counts); if (rc) return rc;
    return provenance_batch(c, c->next_lane++ % c->lanes.size(), poses, n_frames, d_imgs_u8, d_labels, d_faces, d_echoes, echo_stride, d_echo_counts,
                            stream_of(c, stream));
}

int rr_simulate_provenance(rr_ctx* c, const float pose[7], uint8_t* out_u8, uint32_t* out_labels, uint32_t* out_faces, rr_echo_src* out_echoes,
                           size_t echo_stride, uint32_t* out_echo_counts)
{
    int rc = check_provenance(c, "rr_simulate_provenance", pose, 1, out_u8, out_echoes, echo_stride, out_echo_counts); if (rc) return rc;
    Lane& L = c->lanes[0];
    rc = host_lane(c, L); if (rc) return rc;
    rc = ensure_prov_buffers(c, L); if (rc) return rc;
    const size_t A = (size_t)c->cfg.n_angles, npx = A * (size_t)c->cfg.n_cells;
    const size_t d_stride = out_echoes ? std::min(echo_stride, (size_t)L.prov_cap) : 0;      // the device-side row: as long as the caller's, and no longer than a list can get
    Stage st(c, L.stage, c->stream); uint32_t *d_labels, *d_faces, *d_counts; rr_echo_src* d_echoes;
    st.out(out_u8, L.slot[0].img.p, npx);
    RR_HIP(c, st.hold(out_labels, npx, d_labels));
    RR_HIP(c, st.hold(out_faces, npx, d_faces));
    RR_HIP(c, st.hold(out_echo_counts, A, d_counts));
    RR_HIP(c, st.hold_rows(out_echoes, A, d_stride, echo_stride, out_echo_counts, d_echoes));
    rc = provenance_batch(c, 0, pose, 1, L.slot[0].img.p, d_labels, d_faces, d_echoes, d_stride, d_counts, c->stream); if (rc) return rc;
    return commit_lane(c, st, L);
}

int rr_simulate_batch_paths_device(rr_ctx* c, const float* poses, int n_frames, uint8_t* d_imgs_u8, rr_wave_rec* d_waves, size_t wave_stride,
                                   uint32_t* d_wave_counts, uint32_t* d_pass_counts, unsigned flags, void* stream)
{
    int rc = check_paths(c, "rr_simulate_batch_paths_device", poses, n_frames, d_imgs_u8, d_waves, wave_stride, d_wave_counts, flags, false); if (rc) return rc;
    return paths_batch(c, c->next_lane++ % c->lanes.size(), poses, n_frames, d_imgs_u8, d_waves, wave_stride, d_wave_counts, d_pass_counts, flags,
                       stream_of(c, stream));
}

int rr_simulate_paths(rr_ctx* c, const float pose[7], uint8_t* out_u8, rr_wave_rec* out_waves, size_t wave_stride, uint32_t* out_wave_counts,
                      uint32_t* out_pass_counts, unsigned flags)
{
    int rc = check_paths(c, "rr_simulate_paths", pose, 1, out_u8, out_waves, wave_stride, out_wave_counts, flags, true); if (rc) return rc;
    Lane& L = c->lanes[0];
    rc = host_lane(c, L); if (rc) return rc;
    const size_t A = (size_t)c->cfg.n_angles, npx = A * (size_t)c->cfg.n_cells;
    // the device-side row: as long as the caller's, and no longer than a list can get (every pass' wave bound)
    size_t longest = 0;
    { const long n_beam = (long)(c->beams.size() / 3); long w = n_beam;
      for (int p = 0; p < c->cfg.n_reflections; p++) { longest += (size_t)std::min<long>(w, L.buf_cap); w = std::min<long>(2 * w, L.buf_cap); } }
    const size_t d_stride = out_waves ? std::max<size_t>(1, std::min(wave_stride, longest)) : 0;
    Stage st(c, L.stage, c->stream); uint32_t *d_counts, *d_passes; rr_wave_rec* d_waves;
    st.out(out_u8, L.slot[0].img.p, npx);
    RR_HIP(c, st.hold(out_wave_counts, A, d_counts));
    RR_HIP(c, st.hold(out_pass_counts, A * RR_WAVES_MAX_PASSES, d_passes));
    RR_HIP(c, st.hold_rows(out_waves, A, d_stride, wave_stride, out_wave_counts, d_waves));
    rc = paths_batch(c, 0, pose, 1, L.slot[0].img.p, d_waves, d_stride, d_counts, d_passes, flags, c->stream); if (rc) return rc;
    return commit_lane(c, st, L);
}

int rr_simulate_batch_doppler_device(rr_ctx* c, const float* poses, int n_frames, const float* sensor_vel, float gain, uint8_t* d_imgs_u8,
                                     float* d_echo_vel, size_t echo_stride, uint32_t* d_echo_counts, int32_t* d_echo_cells, float* d_vel_img, void* stream)
{
    int rc = check_doppler(c, "rr_simulate_batch_doppler_device", poses, n_frames, sensor_vel, gain, d_imgs_u8, d_echo_vel, d_echo_cells, echo_stride,
                           d_echo_counts, d_vel_img); if (rc) return rc;
    return doppler_batch(c, c->next_lane++ % c->lanes.size(), poses, n_frames, sensor_vel, gain, d_imgs_u8, nullptr, d_echo_vel, echo_stride, d_echo_counts,
                         d_echo_cells, d_vel_img, stream_of(c, stream));
}

int rr_simulate_doppler(rr_ctx* c, const float pose[7], const float sensor_vel[3], float gain, uint8_t* out_u8, float* out_f32, float* out_echo_vel,
                        size_t echo_stride, uint32_t* out_echo_counts, int32_t* out_echo_cells, float* out_vel_img)
{
    int rc = check_doppler(c, "rr_simulate_doppler", pose, 1, sensor_vel, gain, out_u8, out_echo_vel, out_echo_cells, echo_stride, out_echo_counts, out_vel_img); if (rc) return rc;
    Lane& L = c->lanes[0];
    rc = host_lane(c, L, out_f32 != nullptr); if (rc) return rc;
    rc = ensure_prov_buffers(c, L); if (rc) return rc;
    const size_t A = (size_t)c->cfg.n_angles, npx = A * (size_t)c->cfg.n_cells;
    const size_t d_stride = (out_echo_vel || out_echo_cells) ? std::min(echo_stride, (size_t)L.prov_cap) : 0;      // the device-side rows: as long as the caller's, and no longer than a list can get
    Stage st(c, L.stage, c->stream); float *d_f32, *d_vel_img, *d_vel; uint32_t* d_counts; int32_t* d_cells;
    st.out(out_u8, L.slot[0].img.p, npx);
    RR_HIP(c, st.hold(out_f32, npx, d_f32));
    RR_HIP(c, st.hold(out_vel_img, npx, d_vel_img));
    RR_HIP(c, st.hold(out_echo_counts, A, d_counts));
    RR_HIP(c, st.hold_rows(out_echo_vel, A, d_stride, echo_stride, out_echo_counts, d_vel));
    RR_HIP(c, st.hold_rows(out_echo_cells, A, d_stride, echo_stride, out_echo_counts, d_cells));
    rc = doppler_batch(c, 0, pose, 1, sensor_vel, gain, L.slot[0].img.p, d_f32, d_vel, d_stride, d_counts, d_cells, d_vel_img, c->stream); if (rc) return rc;
    return commit_lane(c, st, L);
}

int rr_debug_labels(rr_ctx* c, int n_seg, int az_begin, const rr_echo_src* echoes, const uint32_t* counts, size_t stride, uint32_t* out_labels,
                    uint32_t* out_faces)
{
    if (!c) return -1;
    if (!c->have_cfg) return fail(c, -2, "rr_set_config has not been called");
    const rr_config& g = c->cfg;
    if (n_seg < 1 || az_begin < 0 || az_begin > g.n_angles - n_seg) return fail(c, -3, "rr_debug_labels: azimuth block out of bounds");
    if (!counts || !out_labels || !out_faces || (stride > 0 && !echoes)) return fail(c, -3, "rr_debug_labels: null buffer");
    if (g.n_cells > kLabelMaxCells) return fail(c, -3, "rr_debug_labels: n_cells exceeds RR_LABEL_MAX_CELLS (8192)");
    for (int k = 0; k < n_seg; k++) if (counts[k] > stride) return fail(c, -3, "rr_debug_labels: a count exceeds stride");
    RR_HIP(c, hipSetDevice(c->device));
    int rc = upload_tables(c); if (rc) return rc;
    const size_t S = (size_t)n_seg, px = S * (size_t)g.n_cells;
    DevBuf<EchoSrc> d_e; DevBuf<uint32_t> d_n, d_l, d_f;
    RR_HIP(c, d_e.ensure(S * stride)); RR_HIP(c, d_n.ensure(S)); RR_HIP(c, d_l.ensure(px)); RR_HIP(c, d_f.ensure(px));
    if (stride) RR_HIP(c, hipMemcpy(d_e.p, echoes, S * stride * sizeof(rr_echo_src), hipMemcpyHostToDevice));
    RR_HIP(c, hipMemcpy(d_n.p, counts, S * sizeof(uint32_t), hipMemcpyHostToDevice));
    const bool den = !c->smear.empty() && g.signal_denoising > 0;
    launch_label(d_e.p, d_n.p, stride, n_seg, g.n_cells, den ? (int)c->smear.size() : 1, den ? c->smear_mode : 0, den ? c->d_smear.p : nullptr, d_l.p, d_f.p,
                 c->stream);
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipStreamSynchronize(c->stream));
    RR_HIP(c, hipMemcpy(out_labels, d_l.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost));
    RR_HIP(c, hipMemcpy(out_faces, d_f.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
