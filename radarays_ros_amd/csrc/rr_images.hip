// rr_images.hip -- the C ABI's image entry points: images in, records / points / images out.  PSNR scores and metrics against a reference image
// (rr_metrics.hip), azimuth registration (rr_align.hip), translation registration (rr_shift.hip), place recognition (rr_place.hip), point clouds and Cartesian images (rr_detect.hip), sweep compensation (rr_deskew.hip), scan matching (rr_icp.hip), the likelihood field (rr_field.hip), occupancy mapping (rr_occupancy.hip), the particle filter step (rr_filter.hip), map refinement (rr_refine.hip), the beam model (rr_cast.hip), mesh maps (rr_slice.hip), connected components (rr_components.hip), correlative scan matching (rr_correlate.hip), pose-graph optimisation (rr_graph.hip), object annotations (rr_notes.hip): each in a device form, which runs on the
// caller's buffers and stream, and a host form, which drains c->stream and makes its round trip through a Stage over the context's pool (rr_stage.h).
#include "rr_grid.h"
#include "rr_stage.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace rr {
namespace {

// the compare and align forms work through their images 64 at a time: scratch of 256 KB of histogram (kBins words) or one curve per image of a chunk
constexpr size_t kChunk = 64, kBins = 65536;

// skimage.metrics.peak_signal_noise_ratio for uint8 (scripts/radaray_opti.py:196): data_range 255,
// err = mean of the squared differences in f64 (exact here: an integer sum below 2^53), 10 log10(255^2 / err)
double psnr_of(uint64_t sse, size_t npx)
{
    const double err = (double)sse / (double)npx;
    return err > 0.0 ? 10.0 * std::log10((255.0 * 255.0) / err) : INFINITY;
}

// ---- refusals ---------------------------------------------------------------------------------------------------------
// what every check below opens with: a context with a config, the caller's buffers, a count in range
int check_images(rr_ctx* c, const std::string& w, bool have_buffers, const char* buffers, const char* count, int n, int n_max)
{
    if (!c) return -1;
    if (!c->have_cfg) return fail(c, -2, "rr_set_config has not been called");
    if (!have_buffers) return fail(c, -3, w + ": null " + buffers);
    if (n < 1 || n > n_max) return fail(c, -3, w + ": " + count + " must be 1.." + std::to_string(n_max));
    return 0;
}

// the refusals of rr_align_images_device / rr_align_images / rr_simulate_batch_align
int check_align(rr_ctx* c, const char* who, const void* imgs, int n_images, int n_max, const void* ref, int cell_begin, int cell_end, const void* out)
{
    const std::string w(who);
    int rc = check_images(c, w, imgs && ref && out, "buffer", "n_images", n_images, n_max); if (rc) return rc;
    if (cell_begin < 0 || cell_end > c->cfg.n_cells || cell_begin >= cell_end)
        return fail(c, -3, w + ": the cell window [" + std::to_string(cell_begin) + ", " + std::to_string(cell_end) + ") must be non-empty and inside 0.." +
                               std::to_string(c->cfg.n_cells));
    if ((long long)(cell_end - cell_begin) * c->cfg.n_angles > (1ll << 23))
        return fail(c, -3, w + ": a window of more than 2^23 pixels");
    return 0;
}

// the refusals of rr_shift_images_device / rr_shift_images / rr_simulate_batch_shift: no config is needed, the shape comes with the call
int check_shift(rr_ctx* c, const char* who, const void* imgs, int n_images, int n_max, const void* ref, int H, int W, int S, const void* out)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(imgs && ref && out)) return fail(c, -3, w + ": null buffer");
    if (n_images < 1 || n_images > n_max) return fail(c, -3, w + ": n_images must be 1.." + std::to_string(n_max));
    if (H < 1 || H > 8192 || W < 1 || W > 8192) return fail(c, -3, w + ": height and width must be 1..8192");
    if (S < 0 || S > 64) return fail(c, -3, w + ": max_shift must be 0..64");
    if (H <= 2 * S || W <= 2 * S)
        return fail(c, -3, w + ": the image (" + std::to_string(H) + " x " + std::to_string(W) + ") leaves no template window at max_shift " + std::to_string(S));
    if ((long long)(H - 2 * S) * (W - 2 * S) > (1ll << 23)) return fail(c, -3, w + ": a template window of more than 2^23 pixels");
    return 0;
}

int check_detect(rr_ctx* c, const char* who, const void* imgs, int n_frames, const rr_detect_config* d, const void* points,
                 int max_points, const void* offsets)
{
    const std::string w(who);
    int rc = check_images(c, w, imgs != nullptr, "images", "n_frames", n_frames, 65535); if (rc) return rc;
    if (!d) return fail(c, -3, w + ": null config");
    if (!offsets) return fail(c, -3, w + ": null offsets");
    if (max_points < 0) return fail(c, -3, w + ": max_points must be >= 0");
    if (max_points > 0 && !points) return fail(c, -3, w + ": null points with max_points > 0");
    const int n_cells = c->cfg.n_cells;
    if (d->method != 0 && d->method != 1) return fail(c, -3, w + ": method must be 0 (CA-CFAR) or 1 (k-strongest)");
    if (d->guard_cells < 0 || d->guard_cells > 1024) return fail(c, -3, w + ": guard_cells must be 0..1024");
    if (d->train_cells < 1 || d->train_cells > 1024) return fail(c, -3, w + ": train_cells must be 1..1024");
    if (d->k < 1 || d->k > n_cells) return fail(c, -3, w + ": k must be 1..n_cells (" + std::to_string(n_cells) + ")");
    if (d->min_intensity < 0 || d->min_intensity > 255) return fail(c, -3, w + ": min_intensity must be 0..255");
    if (d->min_bin < 0 || d->min_bin >= n_cells) return fail(c, -3, w + ": min_bin must be 0..n_cells-1");
    if (!(std::isfinite(d->cfar_scale) && d->cfar_scale >= 0.0f)) return fail(c, -3, w + ": cfar_scale must be finite and >= 0");
    return 0;
}

int check_cartesian(rr_ctx* c, const char* who, const void* imgs, int n_frames, const rr_cartesian_config* k, const void* out)
{
    const std::string w(who);
    int rc = check_images(c, w, imgs != nullptr, "images", "n_frames", n_frames, 65535); if (rc) return rc;
    if (!k) return fail(c, -3, w + ": null config");
    if (!out) return fail(c, -3, w + ": null output");
    if (k->width < 1 || k->width > 8192) return fail(c, -3, w + ": width must be 1..8192");
    if (k->interpolation != 0 && k->interpolation != 1) return fail(c, -3, w + ": interpolation must be 0 (nearest) or 1 (bilinear)");
    if (!(std::isfinite(k->pixel_size) && k->pixel_size > 0.0f)) return fail(c, -3, w + ": pixel_size must be finite and > 0");
    if (c->cfg.theta_inc == 0.0f) return fail(c, -3, w + ": the config's theta_inc is 0");
    return 0;
}

// the refusals the sweep compensation calls share; a device table is read with 16-byte loads, a host table is staged
int check_sweep(rr_ctx* c, const std::string& w, bool have_buffers, int n_frames, const void* table, bool device)
{
    int rc = check_images(c, w, have_buffers && table, "buffer", "n_frames", n_frames, 65535); if (rc) return rc;
    if (device && (uintptr_t)table % 16 != 0) return fail(c, -3, w + ": the table must be 16-byte aligned");
    return 0;
}

int check_sweep_table(rr_ctx* c, const char* who, const void* az, const void* ref, float gain, int n_frames, const void* table, bool device)
{
    const std::string w(who);
    int rc = check_sweep(c, w, az && ref, n_frames, table, device); if (rc) return rc;
    if (!std::isfinite(gain)) return fail(c, -3, w + ": gain must be finite");
    return 0;
}

int check_compensate(rr_ctx* c, const char* who, const void* points, const void* offsets, int n_frames, int max_points, const void* table,
                     const void* out, bool device)
{
    const std::string w(who);
    int rc = check_sweep(c, w, offsets && (max_points <= 0 || (points && out)), n_frames, table, device); if (rc) return rc;
    if (max_points < 0) return fail(c, -3, w + ": max_points must be >= 0");
    return 0;
}

int check_cartesian_sweep(rr_ctx* c, const char* who, const void* imgs, int n_frames, const rr_cartesian_config* k, const void* table, int iterations,
                          const void* out, bool device)
{
    const std::string w(who);
    int rc = check_cartesian(c, who, imgs, n_frames, k, out); if (rc) return rc;
    rc = check_sweep(c, w, true, n_frames, table, device); if (rc) return rc;
    if (iterations < 1 || iterations > 8) return fail(c, -3, w + ": iterations must be 1..8");
    if ((size_t)c->cfg.n_angles * sizeof(rr_sweep_rec) > 65536)
        return fail(c, -3, w + ": n_angles * 32 exceeds 65536: a frame's records do not fit in LDS");
    return 0;
}

// the refusals of rr_register_points_device / rr_register_points
int check_icp(rr_ctx* c, const char* who, const void* points, const void* offsets, int n_frames, int max_points, const void* tgt, bool have_count,
              int max_tgt, float gate, int iterations, const void* recs)
{
    const std::string w(who);
    const bool sizes_ok = max_points >= 0 && max_points <= 65536 && max_tgt >= 0 && max_tgt <= 65536;
    int rc = check_images(c, w, offsets && have_count && recs && (!sizes_ok || ((max_points == 0 || points) && (max_tgt == 0 || tgt))), "buffer",
                          "n_frames", n_frames, 65535); if (rc) return rc;
    if (!sizes_ok) return fail(c, -3, w + ": max_points and max_tgt must be 0..65536");
    if (iterations < 0 || iterations > 64) return fail(c, -3, w + ": iterations must be 0..64");
    if (!(std::isfinite(gate) && gate > 0.0f)) return fail(c, -3, w + ": gate must be finite and > 0");
    return 0;
}

// the refusals of rr_surfels_scratch_bytes and, behind it, of the surface-point calls: the shape alone
const char* bad_surfels_shape(int n_frames, const rr_surfel_config* g)
{
    if (!g) return "null config";
    if (n_frames < 1 || n_frames > 65535) return "n_frames must be 1..65535";
    if (!(std::isfinite(g->cell) && g->cell > 0.0f && g->cell <= 16.0f) || rintf(g->cell * 256.0f) < 1.0f || rintf(g->cell * 256.0f) > 4096.0f)
        return "cell must give rintf(cell * 256) in 1..4096";
    if (g->width < 1 || g->width > 1024) return "width must be 1..1024";
    if (g->min_points < 2 || g->min_points > 65536) return "min_points must be 2..65536";
    if (!(g->max_ratio >= 0.0f && g->max_ratio <= 1.0f)) return "max_ratio must be 0..1";
    for (int k = 0; k < 4; k++) if (g->reserved_[k] != 0) return "reserved_ must be 0";
    return nullptr;
}

// the refusals of rr_surface_points_device / rr_surface_points: the config gives n_angles, the offsets' stride
int check_surfels(rr_ctx* c, const std::string& w, const void* points, const void* offsets, int n_frames, int max_points, const rr_surfel_config* g,
                  const void* surfels, int max_surfels, const void* counts)
{
    const bool sizes_ok = max_points >= 0 && max_points <= 65536;
    int rc = check_images(c, w, offsets && counts && (!sizes_ok || max_points == 0 || points), "buffer", "n_frames", n_frames, 65535); if (rc) return rc;
    if (!sizes_ok) return fail(c, -3, w + ": max_points must be 0..65536");
    if (const char* bad = bad_surfels_shape(n_frames, g)) return fail(c, -3, w + ": " + bad);
    if (max_surfels < 0 || max_surfels > (1 << 20)) return fail(c, -3, w + ": max_surfels must be 0..1048576");
    if (!surfels != (max_surfels == 0)) return fail(c, -3, w + ": the records come with max_surfels > 0 and only with it");
    return 0;
}

// the refusals of rr_graph_plan_bytes / rr_graph_scratch_bytes and, behind them, of the pose-graph calls: the shape alone
const char* bad_graph_shape(int n_nodes, int n_edges)
{
    if (n_nodes < 1 || n_nodes > (1 << 20)) return "n_nodes must be 1..1048576";
    if (n_edges < 0 || n_edges > (1 << 22)) return "n_edges must be 0..4194304";
    return nullptr;
}

const char* bad_graph_config(const rr_graph_config* g)
{
    if (!g) return "null config";
    if (g->iterations < 0 || g->iterations > 256) return "iterations must be 0..256";
    if (g->cg_iterations < 0 || g->cg_iterations > 1024) return "cg_iterations must be 0..1024";
    if (!(std::isfinite(g->lambda) && g->lambda >= 0.0)) return "lambda must be finite and >= 0";
    if (!(std::isfinite(g->robust_k) && g->robust_k >= 0.0)) return "robust_k must be finite and >= 0";
    if (g->reserved_[0] != 0 || g->reserved_[1] != 0) return "reserved_ must be 0";
    return nullptr;
}

// the refusals of rr_graph_plan_device / rr_graph_plan: no config of the radar is needed
int check_graph_plan(rr_ctx* c, const std::string& w, const void* edges, int n_nodes, int n_edges, const void* plan, size_t plan_bytes)
{
    if (!c) return -1;
    if (const char* bad = bad_graph_shape(n_nodes, n_edges)) return fail(c, -3, w + ": " + bad);
    if (!plan || (n_edges > 0 && !edges)) return fail(c, -3, w + ": null buffer");
    const size_t need = graph_plan_bytes((size_t)n_nodes, (size_t)n_edges);
    if (plan_bytes < need) return fail(c, -3, w + ": plan of " + std::to_string(plan_bytes) + " bytes, the call needs " + std::to_string(need));
    return 0;
}

// the refusals of rr_optimize_graph_device / rr_optimize_graph
int check_graph(rr_ctx* c, const std::string& w, const void* states, const void* fixed, const void* edges, int n_nodes, int n_edges, const void* plan,
                const rr_graph_config* g, const void* recs)
{
    if (!c) return -1;
    if (const char* bad = bad_graph_shape(n_nodes, n_edges)) return fail(c, -3, w + ": " + bad);
    if (const char* bad = bad_graph_config(g)) return fail(c, -3, w + ": " + bad);
    if (!states || !fixed || !plan || !recs || (n_edges > 0 && !edges)) return fail(c, -3, w + ": null buffer");
    return 0;
}

// the refusals the likelihood-field and the occupancy calls share: the shape and the place of a grid within their stated ranges
int check_grid_shape(rr_ctx* c, const std::string& w, const rr_field_config* g)
{
    if (!g) return fail(c, -3, w + ": null config");
    if (g->width < 1 || g->width > kGridMaxSide || g->height < 1 || g->height > kGridMaxSide)
        return fail(c, -3, w + ": width and height must be 1.." + std::to_string(kGridMaxSide));
    if (!(std::isfinite(g->cell) && g->cell > 0.0f)) return fail(c, -3, w + ": cell must be finite and > 0");
    if (!(std::isfinite(g->x0) && std::isfinite(g->y0))) return fail(c, -3, w + ": x0 and y0 must be finite");
    return 0;
}

// ... what the calls that read a distance table ask on top: the saturation (the ray calls stop here: they ignore the gate, so any value passes)
int check_dist_grid(rr_ctx* c, const std::string& w, const rr_field_config* g)
{
    int rc = check_grid_shape(c, w, g); if (rc) return rc;
    if (g->max_dist < 1 || g->max_dist > kGridMaxDist) return fail(c, -3, w + ": max_dist must be 1.." + std::to_string(kGridMaxDist));
    return 0;
}

// ... and what the likelihood-field and refinement calls ask on top of that: the gate
int check_field_grid(rr_ctx* c, const std::string& w, const rr_field_config* g)
{
    int rc = check_dist_grid(c, w, g); if (rc) return rc;
    if (g->gate < 0 || g->gate > g->max_dist) return fail(c, -3, w + ": gate must be 0..max_dist");
    return 0;
}

// the refusals of rr_rasterize_points_device / rr_rasterize_points: the config gives n_angles, the offsets' stride
int check_rasterize(rr_ctx* c, const char* who, const void* points, const void* offsets, int n_frames, int max_points, const void* states,
                    const rr_field_config* g, const void* occ)
{
    const std::string w(who);
    const bool sizes_ok = max_points >= 0 && max_points <= 65536;
    int rc = check_images(c, w, offsets && occ && (!sizes_ok || max_points == 0 || points), "buffer", "n_frames", n_frames, 65535); if (rc) return rc;
    if (!sizes_ok) return fail(c, -3, w + ": max_points must be 0..65536");
    if ((uintptr_t)states % 8 != 0) return fail(c, -3, w + ": the states must be 8-byte aligned");
    return check_field_grid(c, w, g);
}

// the refusals of rr_distance_field_device / rr_distance_field: no config is needed, the shape comes with the call
int check_distance_field(rr_ctx* c, const char* who, const void* occ, int threshold, const rr_field_config* g, const void* field)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(occ && field)) return fail(c, -3, w + ": null buffer");
    if (threshold < 1 || threshold > 255) return fail(c, -3, w + ": threshold must be 1..255");
    if (occ == field) return fail(c, -3, w + ": the field must not alias the occupancy grid");
    return check_field_grid(c, w, g);
}

// the refusals of rr_score_poses_device / rr_score_poses: no config is needed either
int check_score_poses(rr_ctx* c, const char* who, const void* points, bool have_count, int max_points, const void* states, int n_hyp, const void* field,
                      const rr_field_config* g, const void* recs)
{
    if (!c) return -1;
    const std::string w(who);
    const bool sizes_ok = max_points >= 0 && max_points <= 65536;
    if (!(have_count && states && field && recs && (!sizes_ok || max_points == 0 || points))) return fail(c, -3, w + ": null buffer");
    if (!sizes_ok) return fail(c, -3, w + ": max_points must be 0..65536");
    if (n_hyp < 1 || n_hyp > (1 << 22)) return fail(c, -3, w + ": n_hyp must be 1..2^22");
    if ((uintptr_t)states % 4 != 0 || (uintptr_t)recs % 8 != 0) return fail(c, -3, w + ": d_states must be 4-byte and d_recs 8-byte aligned");
    return check_field_grid(c, w, g);
}

// the refusals of rr_occupancy_update_device / rr_occupancy_update: the config gives the polar geometry; max_dist and gate of the grid are ignored
int check_occupancy_update(rr_ctx* c, const char* who, const void* points, const void* offsets, int n_frames, int max_points, const void* states,
                           const rr_field_config* g, const rr_occupancy_config* o, bool have_profile, const void* profile, const void* evidence)
{
    const std::string w(who);
    const bool sizes_ok = max_points >= 0 && max_points <= 65536;
    int rc = check_images(c, w, offsets && have_profile && evidence && (!sizes_ok || max_points == 0 || points), "buffer", "n_frames", n_frames, 65535);
    if (rc) return rc;
    if (!sizes_ok) return fail(c, -3, w + ": max_points must be 0..65536");
    if ((uintptr_t)states % 8 != 0) return fail(c, -3, w + ": the states must be 8-byte aligned");
    if ((uintptr_t)profile % 4 != 0 || (uintptr_t)evidence % 4 != 0) return fail(c, -3, w + ": the profile and the evidence must be 4-byte aligned");
    rc = check_grid_shape(c, w, g); if (rc) return rc;
    if (!o) return fail(c, -3, w + ": null occupancy config");
    const int n_cells = c->cfg.n_cells;
    if (o->l_hit < 1 || o->l_hit > 127) return fail(c, -3, w + ": l_hit must be 1..127");
    if (o->l_free < 0 || o->l_free > 127) return fail(c, -3, w + ": l_free must be 0..127");
    if (o->margin_bins < 0 || o->margin_bins > n_cells) return fail(c, -3, w + ": margin_bins must be 0..n_cells (" + std::to_string(n_cells) + ")");
    if (o->max_free_bin < 0 || o->max_free_bin > n_cells) return fail(c, -3, w + ": max_free_bin must be 0..n_cells (" + std::to_string(n_cells) + ")");
    if (c->cfg.theta_inc == 0.0f) return fail(c, -3, w + ": the config's theta_inc is 0");
    return 0;
}

// the refusals of rr_occupancy_map_device / rr_occupancy_map: no config is needed, the shape comes with the call
int check_occupancy_map(rr_ctx* c, const char* who, const void* evidence, const rr_field_config* g, const void* occ)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(evidence && occ)) return fail(c, -3, w + ": null buffer");
    if ((uintptr_t)evidence % 4 != 0) return fail(c, -3, w + ": the evidence must be 4-byte aligned");
    return check_grid_shape(c, w, g);
}

// the refusals the particle filter calls share: a config within its stated ranges, particle and draw counts in 1..2^22
int check_filter_config(rr_ctx* c, const std::string& w, const rr_filter_config* f, int n, int n_out)
{
    if (!f) return fail(c, -3, w + ": null config");
    if (n < 1 || n > (1 << 22) || n_out < 1 || n_out > (1 << 22)) return fail(c, -3, w + ": n and n_out must be 1..2^22");
    if (f->quantum < 1 || f->quantum > (1u << 31)) return fail(c, -3, w + ": quantum must be 1..2^31");
    if (f->n_table < 1 || f->n_table > 4096) return fail(c, -3, w + ": n_table must be 1..4096");
    if (f->phase >= (1u << 24)) return fail(c, -3, w + ": phase must be 0..2^24 - 1");
    if (!(std::isfinite(f->sigma_xy) && f->sigma_xy >= 0.0f && std::isfinite(f->sigma_t) && f->sigma_t >= 0.0f))
        return fail(c, -3, w + ": sigma_xy and sigma_t must be finite and >= 0");
    if (f->reserved != 0) return fail(c, -3, w + ": reserved must be 0");
    return 0;
}

// the refusals of rr_filter_resample_device / rr_filter_resample: no config of the radar is needed
int check_filter_resample(rr_ctx* c, const char* who, const void* recs, int n, const void* table, int n_out, const rr_filter_config* f, const void* cum,
                          const void* ancestors, const void* summary)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(recs && table && cum && ancestors && summary)) return fail(c, -3, w + ": null buffer");
    int rc = check_filter_config(c, w, f, n, n_out); if (rc) return rc;
    if ((uintptr_t)recs % 8 != 0 || (uintptr_t)cum % 8 != 0 || (uintptr_t)summary % 8 != 0 || (uintptr_t)ancestors % 4 != 0 || (uintptr_t)table % 2 != 0)
        return fail(c, -3, w + ": d_recs, d_cum and d_summary must be 8-byte, d_ancestors 4-byte and d_table 2-byte aligned");
    return 0;
}

// the refusals of rr_filter_move_device / rr_filter_move
int check_filter_move(rr_ctx* c, const char* who, const float* in, int n, const void* ancestors, int n_out, float Dc, float Ds, float dx, float dy,
                      const rr_filter_config* f, const float* out, size_t align /*of the states: 16 on the device, 4 on the host*/)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(in && out)) return fail(c, -3, w + ": null buffer");
    int rc = check_filter_config(c, w, f, n, n_out); if (rc) return rc;
    if (!ancestors && n_out > n) return fail(c, -3, w + ": n_out must not exceed n without ancestors");
    if (!(std::isfinite(Dc) && std::isfinite(Ds) && std::isfinite(dx) && std::isfinite(dy))) return fail(c, -3, w + ": the increment must be finite");
    if ((uintptr_t)in % align != 0 || (uintptr_t)out % align != 0 || (uintptr_t)ancestors % 4 != 0)
        return fail(c, -3, w + ": the states must be " + std::to_string(align) + "-byte and the ancestors 4-byte aligned");
    if (in < out + 4 * (size_t)n_out && out < in + 4 * (size_t)n) return fail(c, -3, w + ": states_out must not overlap states_in");
    return 0;
}

// the refusals of rr_nearest_field_device / rr_nearest_field: no config is needed, the shape comes with the call
int check_nearest_field(rr_ctx* c, const char* who, const void* occ, int threshold, const rr_field_config* g, const void* nearest)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(occ && nearest)) return fail(c, -3, w + ": null buffer");
    if (threshold < 1 || threshold > 255) return fail(c, -3, w + ": threshold must be 1..255");
    if (occ == nearest) return fail(c, -3, w + ": the nearest-cell table must not alias the occupancy grid");
    if ((uintptr_t)nearest % 4 != 0) return fail(c, -3, w + ": the nearest-cell table must be 4-byte aligned");
    return check_field_grid(c, w, g);
}

// the refusals of rr_refine_poses_device / rr_refine_poses: no config is needed either; the grid must lie within +-8192 m (|P|, |Q| <= 2^21)
int check_refine_poses(rr_ctx* c, const char* who, const void* points, bool have_count, int max_points, const void* init, int n_hyp,
                       const void* nearest, const rr_field_config* g, int iterations, const void* recs)
{
    if (!c) return -1;
    const std::string w(who);
    const bool sizes_ok = max_points >= 0 && max_points <= 65536;
    if (!(have_count && init && nearest && recs && (!sizes_ok || max_points == 0 || points))) return fail(c, -3, w + ": null buffer");
    if (!sizes_ok) return fail(c, -3, w + ": max_points must be 0..65536");
    if (n_hyp < 1 || n_hyp > (1 << 22)) return fail(c, -3, w + ": n_hyp must be 1..2^22");
    if (iterations < 0 || iterations > 64) return fail(c, -3, w + ": iterations must be 0..64");
    if ((uintptr_t)init % 8 != 0 || (uintptr_t)recs % 8 != 0 || (uintptr_t)nearest % 4 != 0)
        return fail(c, -3, w + ": init and recs must be 8-byte and the nearest-cell table 4-byte aligned");
    int rc = check_field_grid(c, w, g); if (rc) return rc;
    const double x0 = (double)g->x0, y0 = (double)g->y0, cell = (double)g->cell;
    const double ext[4] = {x0, y0, x0 + (double)g->width * cell, y0 + (double)g->height * cell};
    for (double e : ext)
        if (!(std::fabs(e) < 8192.0)) return fail(c, -3, w + ": the grid must lie within +-8192 m");
    return 0;
}

// the refusals of rr_scan_profile_device / rr_scan_profile: the config gives the polar geometry; a bin must fit the table's 16 bits
int check_scan_profile(rr_ctx* c, const char* who, const void* points, const void* offsets, int n_frames, int max_points, const void* first_bin)
{
    const std::string w(who);
    const bool sizes_ok = max_points >= 0 && max_points <= 65536;
    int rc = check_images(c, w, offsets && first_bin && (!sizes_ok || max_points == 0 || points), "buffer", "n_frames", n_frames, 65535); if (rc) return rc;
    if (!sizes_ok) return fail(c, -3, w + ": max_points must be 0..65536");
    if (c->cfg.n_cells > 65535) return fail(c, -3, w + ": n_cells must be at most 65535");
    if ((uintptr_t)first_bin % 2 != 0) return fail(c, -3, w + ": the profile must be 2-byte aligned");
    return 0;
}

// the refusals of the two ray calls (rr_cast_map, rr_score_beams and their device forms): `profile` and `recs` are the score form's, `ranges` the
// range form's (the other form passes `true` in their place)
int check_cast(rr_ctx* c, const char* who, bool have_profile, const void* profile, const void* states, int n_hyp, int n_hyp_max, const char* n_hyp_range,
               const void* dirs, const void* field, const rr_field_config* g, const rr_beam_config* b, bool have_out, const void* ranges, const void* recs)
{
    const std::string w(who);
    int rc = check_images(c, w, have_profile && states && dirs && field && have_out, "buffer", "n_hyp", 1, 1); if (rc) return rc;
    if (n_hyp < 1 || n_hyp > n_hyp_max) return fail(c, -3, w + ": n_hyp must be " + n_hyp_range);
    rc = check_dist_grid(c, w, g); if (rc) return rc;
    if (!b) return fail(c, -3, w + ": null beam config");
    const int n_cells = c->cfg.n_cells;
    if (n_cells > 65535) return fail(c, -3, w + ": n_cells must be at most 65535");
    if (b->bin_begin < 0 || b->bin_begin > b->bin_end || b->bin_end > n_cells)
        return fail(c, -3, w + ": 0 <= bin_begin <= bin_end <= n_cells (" + std::to_string(n_cells) + ") must hold");
    if (b->bin_step < 1 || b->bin_step > 64) return fail(c, -3, w + ": bin_step must be 1..64");
    if (b->tol_bins < 0 || b->tol_bins > n_cells) return fail(c, -3, w + ": tol_bins must be 0..n_cells (" + std::to_string(n_cells) + ")");
    if (b->clip_bins < 0 || b->clip_bins > n_cells) return fail(c, -3, w + ": clip_bins must be 0..n_cells (" + std::to_string(n_cells) + ")");
    if (b->reserved_[0] != 0 || b->reserved_[1] != 0 || b->reserved_[2] != 0) return fail(c, -3, w + ": reserved must be 0");
    if ((uintptr_t)states % 4 != 0 || (uintptr_t)dirs % 4 != 0 || (uintptr_t)field % 2 != 0 || (uintptr_t)profile % 2 != 0 || (uintptr_t)ranges % 2 != 0 ||
        (uintptr_t)recs % 8 != 0)
        return fail(c, -3, w + ": states and dirs must be 4-byte, the 16-bit tables 2-byte and the records 8-byte aligned");
    return 0;
}

// the refusals of rr_slice_mesh_device / rr_slice_mesh: a mesh, no config of the radar
int check_slice(rr_ctx* c, const char* who, const rr_slice_config* sc, const rr_field_config* g, const void* occ, const void* objects)
{
    if (!c) return -1;
    if (!c->have_mesh) return fail(c, -2, "rr_set_mesh has not been called");
    const std::string w(who);
    if (!sc) return fail(c, -3, w + ": null slice config");
    int rc = check_field_grid(c, w, g); if (rc) return rc;
    if (!occ) return fail(c, -3, w + ": null buffer");
    if (!(std::isfinite(sc->z_lo) && std::isfinite(sc->z_hi) && sc->z_lo <= sc->z_hi)) return fail(c, -3, w + ": z_lo and z_hi must be finite and z_lo <= z_hi");
    if (sc->flags != 0) return fail(c, -3, w + ": flags must be 0");
    if ((uintptr_t)objects % 4 != 0) return fail(c, -3, w + ": the object plane must be 4-byte aligned");
    return 0;
}

// the refusals of rr_components_scratch_bytes and, behind it, of the component calls: the shape alone
const char* bad_components_shape(int n_planes, const rr_components_config* g)
{
    if (!g) return "null config";
    if (n_planes < 1 || n_planes > 65535) return "n_planes must be 1..65535";
    if (g->height < 1 || g->height > 8192 || g->width < 1 || g->width > 8192) return "height and width must be 1..8192";
    if (g->threshold < 1 || g->threshold > 255) return "threshold must be 1..255";
    if (g->connectivity != 4 && g->connectivity != 8) return "connectivity must be 4 or 8";
    if (g->wrap_x != 0 && g->wrap_x != 1) return "wrap_x must be 0 or 1";
    if (g->wrap_x && g->width < 3) return "wrap_x needs width >= 3";
    if (g->min_pixels < 1) return "min_pixels must be >= 1";
    if (g->max_components < 0) return "max_components must be >= 0";
    if (g->reserved_ != 0) return "reserved_ must be 0";
    return nullptr;
}

// the refusals of rr_label_components_device / rr_label_components: no config of the radar and no mesh, the shape comes with the call
int check_components(rr_ctx* c, const char* who, const void* planes, int n_planes, const rr_components_config* g, const void* clean, const void* comps,
                     const void* counts)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(planes && counts)) return fail(c, -3, w + ": null buffer");
    if (const char* bad = bad_components_shape(n_planes, g)) return fail(c, -3, w + ": " + bad);
    if (!comps != (g->max_components == 0)) return fail(c, -3, w + ": the records come with max_components > 0 and only with it");
    const uintptr_t a = (uintptr_t)planes, b = (uintptr_t)clean, bytes = (uintptr_t)n_planes * g->height * g->width;
    if (clean && a < b + bytes && b < a + bytes) return fail(c, -3, w + ": the cleaned plane must not overlap the input");
    return 0;
}

// the refusals of rr_correlate_scratch_bytes and, behind it, of rr_correlate_scan[_device]: the shape of the search alone
const char* bad_correlate_shape(int n_rot, int max_points, const rr_corr_config* k)
{
    if (!k) return "null search config";
    if (n_rot < 1 || n_rot > 4096) return "n_rot must be 1..4096";
    if (max_points < 0 || max_points > 65536) return "max_points must be 0..65536";
    if (k->half_x < 0 || k->half_x > 2047 || k->half_y < 0 || k->half_y > 2047) return "half_x and half_y must be 0..2047";
    if (k->levels < 0 || k->levels > 8) return "levels must be 0..8";
    if (k->capacity < 1 || k->capacity > (1 << 24)) return "capacity must be 1..2^24";
    if (k->reserved_[0] || k->reserved_[1] || k->reserved_[2] || k->reserved_[3]) return "reserved_ must be 0";
    if ((long long)n_rot * (2 * k->half_x + 1) * (2 * k->half_y + 1) >= (1ll << 31)) return "the window holds 2^31 nodes or more";
    return nullptr;
}

// the refusals of rr_field_pyramid_device / rr_field_pyramid: no config is needed, the shape comes with the call
int check_pyramid(rr_ctx* c, const char* who, const void* field, const rr_field_config* g, int levels, const void* pyramid)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(field && pyramid)) return fail(c, -3, w + ": null buffer");
    if (levels < 0 || levels > 8) return fail(c, -3, w + ": levels must be 0..8");
    if ((uintptr_t)field % 2 != 0 || (uintptr_t)pyramid % 2 != 0) return fail(c, -3, w + ": the field and the pyramid must be 2-byte aligned");
    return check_field_grid(c, w, g);
}

// the refusals of rr_correlate_scan_device / rr_correlate_scan
int check_correlate(rr_ctx* c, const char* who, const void* points, bool have_count, int max_points, const void* rot, int n_rot, const void* pyramid,
                    const rr_field_config* g, const rr_corr_config* k, const void* rec, bool device)
{
    if (!c) return -1;
    const std::string w(who);
    const bool sizes_ok = max_points >= 0 && max_points <= 65536;
    if (!(have_count && rot && pyramid && rec && (!sizes_ok || max_points == 0 || points))) return fail(c, -3, w + ": null buffer");
    if (const char* bad = bad_correlate_shape(n_rot, max_points, k)) return fail(c, -3, w + ": " + bad);
    if ((uintptr_t)rot % 4 != 0 || (uintptr_t)pyramid % 2 != 0 || (device && (uintptr_t)rec % 16 != 0))
        return fail(c, -3, w + ": d_rot must be 4-byte, the pyramid 2-byte and the record 16-byte aligned");
    return check_field_grid(c, w, g);
}

// the refusals the annotation calls share: a config (the plane shape) within the limits of the label planes and of the packed azimuth
int check_planes(rr_ctx* c, const std::string& w, bool have_buffers, int n_frames, int n_max)
{
    int rc = check_images(c, w, have_buffers, "buffer", "n_frames", n_frames, n_max); if (rc) return rc;
    if (c->cfg.n_cells > RR_LABEL_MAX_CELLS) return fail(c, -3, w + ": n_cells exceeds RR_LABEL_MAX_CELLS (8192)");
    if (c->cfg.n_angles > 65535) return fail(c, -3, w + ": n_angles must be at most 65535");
    return 0;
}

// the refusals of rr_annotate_labels_device / rr_annotate_labels / rr_simulate_batch_annotations
int check_annotate(rr_ctx* c, const char* who, const void* labels, int n_frames, int n_max, long long n_objects, uint32_t extent_mask, const void* notes,
                   const void* skipped)
{
    const std::string w(who);
    int rc = check_planes(c, w, labels && notes && skipped, n_frames, n_max); if (rc) return rc;
    if (n_objects < 1 || n_objects >= 0xFFFFFF) return fail(c, -3, w + ": n_objects must be 1..2^24 - 2");
    if (extent_mask & ~(RR_NOTE_DIRECT | RR_NOTE_GHOST | RR_NOTE_MULTIPATH))
        return fail(c, -3, w + ": extent_mask must be a mask of RR_NOTE_DIRECT | RR_NOTE_GHOST | RR_NOTE_MULTIPATH");
    return 0;
}

// the refusals of the describe calls: a config (the image shape), then the descriptor's own limits
int check_describe(rr_ctx* c, const char* who, const void* imgs, int n, int n_max, const rr_place_config* p, const void* out)
{
    const std::string w(who);
    int rc = check_images(c, w, imgs && out, "buffer", "n", n, n_max); if (rc) return rc;
    if (!p) return fail(c, -3, w + ": null config");
    if (p->n_rings < 1 || p->n_rings > 64) return fail(c, -3, w + ": n_rings must be 1..64");
    if (p->n_sectors < 4 || p->n_sectors > 128) return fail(c, -3, w + ": n_sectors must be 4..128");
    if (p->n_rings * p->n_sectors > 8192) return fail(c, -3, w + ": n_rings * n_sectors must be at most 8192");
    if (p->cell_begin < 0 || p->cell_end > c->cfg.n_cells || p->cell_begin >= p->cell_end)
        return fail(c, -3, w + ": the cell window [" + std::to_string(p->cell_begin) + ", " + std::to_string(p->cell_end) + ") must be non-empty and inside 0.." +
                               std::to_string(c->cfg.n_cells));
    if (p->n_rings > p->cell_end - p->cell_begin) return fail(c, -3, w + ": more rings than cells in the window");
    if (p->n_sectors > c->cfg.n_angles) return fail(c, -3, w + ": more sectors than image columns");
    return 0;
}

// the refusals of rr_match_descriptors_device / rr_match_descriptors: no config is needed, the shape comes with the call
int check_match(rr_ctx* c, const char* who, const void* query, int n_query, const void* db, int n_db, int R, int S, int top_k, const void* out,
                const void* sse, const void* shift)
{
    if (!c) return -1;
    const std::string w(who);
    if (!(query && db && out)) return fail(c, -3, w + ": null buffer");
    if (n_query < 1 || n_query > 64) return fail(c, -3, w + ": n_query must be 1..64");
    if (n_db < 1 || n_db > (1 << 28)) return fail(c, -3, w + ": n_db must be 1..2^28");
    if (R < 1 || R > 64) return fail(c, -3, w + ": n_rings must be 1..64");
    if (S < 4 || S > 128) return fail(c, -3, w + ": n_sectors must be 4..128");
    if (R * S > 8192) return fail(c, -3, w + ": n_rings * n_sectors must be at most 8192");
    if (top_k < 1 || top_k > 32 || top_k > n_db) return fail(c, -3, w + ": top_k must be 1..min(32, n_db)");
    if (shift && !sse) return fail(c, -3, w + ": the shifts come with the sse matrix: shift without sse");
    return 0;
}

// ---- the steps the forms share ----------------------------------------------------------------------------------------
// the way out of a device form: the launches' error, its records to the host, the stream drained
int records_back(rr_ctx* c, void* rec, const void* d_rec, size_t bytes, hipStream_t s)
{
    RR_HIP(c, hipGetLastError());
    RR_HIP(c, hipMemcpyAsync(rec, d_rec, bytes, hipMemcpyDeviceToHost, s));
    RR_HIP(c, hipStreamSynchronize(s));
    return 0;
}

// The chunked host forms (compare, align, shift, describe): `n` images of `npx` bytes, kChunk at a time through one slot of the stage.
// `chunk(d_imgs, at, m)` runs the device form on the `m` staged images, which drains c->stream, and brings that chunk's surfaces home;
// the forms keep their records in a host vector and write the caller's once every chunk has succeeded
template <typename Chunk>
int in_chunks(rr_ctx* c, Stage& st, const uint8_t* imgs_u8, size_t n, size_t npx, Chunk chunk)
{
    uint8_t* d_imgs;
    RR_HIP(c, st.room(std::min(n, kChunk) * npx, d_imgs));
    for (size_t at = 0; at < n; at += kChunk) {
        const size_t m = std::min(kChunk, n - at);
        RR_HIP(c, st.again(d_imgs, imgs_u8 + at * npx, m * npx));
        const int rc = chunk(d_imgs, at, m); if (rc) return rc;
    }
    return 0;
}

// The per-frame point run on its way up: the offsets [n][n_angles + 1], whose last word of a frame is its total, and of every frame its
// first min(total, max_points) points -- nothing beyond them moves.  `totals` serves the same run on the way down (Stage::out_rows)
int up_points(rr_ctx* c, Stage& st, const rr_radar_point* points, const uint32_t* offsets, size_t n, size_t max_points, std::vector<uint32_t>& totals,
              rr_radar_point*& d_points, uint32_t*& d_offsets)
{
    const size_t A = (size_t)c->cfg.n_angles;
    totals.resize(n);
    for (size_t f = 0; f < n; f++) totals[f] = offsets[f * (A + 1) + A];
    RR_HIP(c, st.up(offsets, n * (A + 1), d_offsets));
    RR_HIP(c, st.up_rows(points, n, max_points, totals.data(), d_points));
    return 0;
}

// what every rr_simulate_batch_* form passes before anything is handed out
auto frame_gate(rr_ctx* c) { return [c] { return report_frame_errors(c); }; }

// ---- the two scan matchers' entry points (rr_icp.hip) ----
// what they differ in besides the target's type: the launcher, the accumulator's size, and the line matcher's one refusal of its own
struct PointMatch {
    static constexpr auto launch = launch_icp;
    static constexpr auto scratch_words = icp_scratch_words;
    static const char* refuse_target(const void*) { return nullptr; }
};
struct LineMatch {
    static constexpr auto launch = launch_register_surfels;
    static constexpr auto scratch_words = line_scratch_words;
    static const char* refuse_target(const void* t) { return (uintptr_t)t % 16 != 0 ? ": the target must be 16-byte aligned" : nullptr; }      // (one 16-byte load per surfel)
};

template <class M, class Target>
int register_device(rr_ctx* c, const std::string& w, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points,
                    const Target* d_tgt, const uint32_t* d_tgt_count, int max_tgt, const double* d_init, float gate, int iterations,
                    rr_icp_rec* d_recs, uint32_t* d_corr, void* stream)
{
    int rc = check_icp(c, w.c_str(), d_points, d_offsets, n_frames, max_points, d_tgt, d_tgt_count != nullptr, max_tgt, gate, iterations, d_recs);
    if (rc) return rc;
    if ((uintptr_t)d_init % 8 != 0 || (uintptr_t)d_recs % 8 != 0) return fail(c, -3, w + ": d_init and d_recs must be 8-byte aligned");
    if (const char* why = M::refuse_target(d_tgt)) return fail(c, -3, w + why);
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    Scratch sc(c->scratch_of(s), s);
    long long* acc;      // the eight or fourteen int64 sums per frame: the call's first launch zeroes what it uses
    RR_HIP(c, sc.room(M::scratch_words((size_t)n_frames), acc));
    M::launch(d_points, d_offsets, n_frames, c->cfg.n_angles, max_points, d_tgt, d_tgt_count, max_tgt, d_init, gate, iterations, d_recs, d_corr, acc, s);
    RR_HIP(c, hipGetLastError());
    return 0;
}

template <class M, class Target>
int register_host(rr_ctx* c, const std::string& w, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points,
                  const Target* tgt, uint32_t tgt_count, int max_tgt, const double* init, float gate, int iterations, rr_icp_rec* recs,
                  uint32_t* corr)
{
    int rc = check_icp(c, w.c_str(), points, offsets, n_frames, max_points, tgt, true, max_tgt, gate, iterations, recs); if (rc) return rc;
    const size_t n = (size_t)n_frames, mp = (size_t)max_points, mt = (size_t)max_tgt;
    for (size_t f = 0; init && f < n; f++) {
        const double h = std::sqrt(init[4 * f] * init[4 * f] + init[4 * f + 1] * init[4 * f + 1]);
        if (!(h > 0.0 && std::isfinite(h))) return fail(c, -3, w + ": an initial state whose (c, s) has a zero or non-finite length");
    }
    RR_HIP(c, hipSetDevice(c->device));
    RR_STAGE(c, st);
    std::vector<uint32_t> totals; rr_radar_point* d_src; Target* d_tgt; uint32_t *d_offs, *d_count, *d_corr; double* d_init; rr_icp_rec* d_recs;
    rc = up_points(c, st, points, offsets, n, mp, totals, d_src, d_offs); if (rc) return rc;
    RR_HIP(c, st.up_rows(tgt, 1, mt, &tgt_count, d_tgt));
    RR_HIP(c, st.up(&tgt_count, 1, d_count));
    RR_HIP(c, st.up(init, n * 4, d_init));
    RR_HIP(c, st.hold(recs, n, d_recs));
    RR_HIP(c, st.hold_rows(corr, n, mp, mp, totals.data(), d_corr));
    RR_HIP(c, hipStreamSynchronize(c->stream));        // (tgt_count is this call's own variable)
    rc = register_device<M>(c, w + "_device", d_src, d_offs, n_frames, max_points, d_tgt, d_count, max_tgt, d_init, gate, iterations, d_recs, d_corr, c->stream);
    if (rc) return rc;
    return st.commit();
}
}  // namespace

// the refusals of rr_compare_images_device / rr_compare_images / rr_simulate_param_sets_metrics
int check_compare(rr_ctx* c, const char* who, const void* imgs, int n_images, const void* ref, uint32_t which, int win_size, const void* out,
                  const void* hist)
{
    const std::string w(who);
    int rc = check_images(c, w, imgs && ref && out, "buffer", "n_images", n_images, 65535); if (rc) return rc;
    const uint32_t all = RR_METRIC_PSNR | RR_METRIC_SSIM | RR_METRIC_INFO;
    if (which == 0 || (which & ~all)) return fail(c, -3, w + ": which must be a non-empty mask of RR_METRIC_PSNR | RR_METRIC_SSIM | RR_METRIC_INFO");
    if (which & RR_METRIC_SSIM) {
        if (win_size < 3 || win_size > 15 || win_size % 2 == 0) return fail(c, -3, w + ": win_size must be odd and in 3..15");
        if (c->cfg.n_cells < win_size || c->cfg.n_angles < win_size)
            return fail(c, -3, w + ": the image (" + std::to_string(c->cfg.n_cells) + " x " + std::to_string(c->cfg.n_angles) + ") is smaller than the window");
    }
    if (hist && !(which & RR_METRIC_INFO)) return fail(c, -3, w + ": a joint histogram buffer needs RR_METRIC_INFO");
    return 0;
}

}  // namespace rr

extern "C" {

int rr_score_images_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n_images, const uint8_t* d_ref_u8, double* out_psnr,
                           uint64_t* out_sse, void* stream)
{
    int rc = check_images(c, "rr_score_images_device", d_imgs_u8 && d_ref_u8 && (out_psnr || out_sse), "buffer", "n_images", n_images, 65535); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "sse words");
    Scratch sc(c->scratch_of(s), s);
    unsigned long long* d_sums;
    RR_HIP(c, sc.room((size_t)n_images, d_sums));
    RR_HIP(c, hipMemsetAsync(d_sums, 0, (size_t)n_images * sizeof(uint64_t), s));
    launch_score(d_imgs_u8, d_ref_u8, npx, n_images, d_sums, s);
    std::vector<uint64_t> sse((size_t)n_images);
    rc = records_back(c, sse.data(), d_sums, sse.size() * sizeof(uint64_t), s); if (rc) return rc;
    for (int k = 0; k < n_images; k++) {
        if (out_sse) out_sse[k] = sse[(size_t)k];
        if (out_psnr) out_psnr[k] = psnr_of(sse[(size_t)k], npx);
    }
    return 0;
}

// ---- images against one reference image: PSNR, SSIM, joint histogram and its entropies (rr_metrics.hip) --------------

int rr_compare_images_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n_images, const uint8_t* d_ref_u8, uint32_t which, int win_size,
                             rr_image_metrics* out, uint32_t* d_joint_hist, void* stream)
{
    int rc = check_compare(c, "rr_compare_images_device", d_imgs_u8, n_images, d_ref_u8, which, win_size, out, d_joint_hist); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    const rr_config& g = c->cfg;
    const size_t npx = (size_t)g.n_cells * g.n_angles, n = (size_t)n_images;
    const bool psnr = which & RR_METRIC_PSNR, ssim = which & RR_METRIC_SSIM, info = which & RR_METRIC_INFO;
    const size_t chunk = std::min(n, kChunk);
    const int n_blocks = ssim ? ssim_blocks(g.n_cells, g.n_angles, win_size) : 0;
    const double ssim_count = ssim ? (double)(g.n_cells - win_size + 1) * (double)(g.n_angles - win_size + 1) : 1.0;
    const bool own_hist = info && !d_joint_hist;
    // the sums, the histograms of one chunk of images, the SSIM partials [image][block], the records: each null where the call has no use for it
    Scratch sc(c->scratch_of(s), s);
    unsigned long long* d_sums; uint32_t* d_hist; double* d_part; rr_image_metrics* d_rec;
    RR_HIP(c, sc.room(psnr ? n : 0, d_sums));
    RR_HIP(c, sc.room(own_hist ? chunk * kBins : 0, d_hist));
    RR_HIP(c, sc.room(ssim ? chunk * (size_t)n_blocks : 0, d_part));
    RR_HIP(c, sc.room(n, d_rec));
    if (psnr) {
        RR_HIP(c, hipMemsetAsync(d_sums, 0, n * sizeof(uint64_t), s));
        launch_score(d_imgs_u8, d_ref_u8, npx, n_images, d_sums, s);
    }
    for (size_t at = 0; at < n; at += kChunk) {
        const int m = (int)std::min(kChunk, n - at);
        const uint8_t* imgs = d_imgs_u8 + at * npx;
        uint32_t* H = !info ? nullptr : d_joint_hist ? d_joint_hist + at * kBins : d_hist;
        if (info) {
            RR_HIP(c, hipMemsetAsync(H, 0, (size_t)m * kBins * sizeof(uint32_t), s));
            launch_joint_hist(imgs, d_ref_u8, npx, m, H, c->metrics_hist, s);
        }
        if (ssim) launch_ssim(imgs, d_ref_u8, g.n_cells, g.n_angles, win_size, m, d_part, s);
        launch_metrics_finish(H, d_part, n_blocks, ssim_count, psnr ? d_sums + at : nullptr, npx, d_rec + at, m, s);
    }
    std::vector<rr_image_metrics> rec(n);
    rc = records_back(c, rec.data(), d_rec, n * sizeof(rr_image_metrics), s); if (rc) return rc;
    for (size_t k = 0; k < n; k++) {
        if (psnr) rec[k].psnr = psnr_of(rec[k].sse, npx);     // the host's log10, as rr_score_images_device: the same bits
        out[k] = rec[k];
    }
    return 0;
}

int rr_compare_images(rr_ctx* c, const uint8_t* imgs_u8, int n_images, const uint8_t* ref_u8, uint32_t which, int win_size,
                      rr_image_metrics* out, uint32_t* joint_hist)
{
    int rc = check_compare(c, "rr_compare_images", imgs_u8, n_images, ref_u8, which, win_size, out, joint_hist); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_images, npx = (size_t)c->cfg.n_cells * c->cfg.n_angles;
    RR_STAGE(c, st);
    uint8_t* d_ref; uint32_t* d_hist = nullptr;
    RR_HIP(c, st.up(ref_u8, npx, d_ref));
    if (joint_hist) RR_HIP(c, st.room(std::min(n, kChunk) * kBins, d_hist));
    std::vector<rr_image_metrics> rec(n);
    rc = in_chunks(c, st, imgs_u8, n, npx, [&](const uint8_t* d_imgs, size_t at, size_t m) {
        // one chunk of the device form, its histograms into this form's own room
        const int rcc = rr_compare_images_device(c, d_imgs, (int)m, d_ref, which, win_size, rec.data() + at, d_hist, c->stream); if (rcc) return rcc;
        if (joint_hist) RR_HIP(c, hipMemcpy(joint_hist + at * kBins, d_hist, m * kBins * sizeof(uint32_t), hipMemcpyDeviceToHost));
        return 0;
    }); if (rc) return rc;
    std::copy(rec.begin(), rec.end(), out);
    return 0;
}

// ---- azimuth registration: the circular cross-correlation over all shifts (rr_align.hip) ------------------------------

int rr_align_images_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n_images, const uint8_t* d_ref_u8, int cell_begin, int cell_end,
                           rr_align_record* out, int64_t* d_xcorr, void* stream)
{
    int rc = check_align(c, "rr_align_images_device", d_imgs_u8, n_images, 65535, d_ref_u8, cell_begin, cell_end, out); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    const rr_config& g = c->cfg;
    const size_t npx = (size_t)g.n_cells * g.n_angles, n = (size_t)n_images, A = (size_t)g.n_angles;
    const size_t chunk = std::min(n, kChunk);
    static_assert(sizeof(long long) == sizeof(int64_t), "curve words");
    // one chunk's curves (when the caller gives no buffer) and sums, the records
    Scratch sc(c->scratch_of(s), s);
    long long* d_curve; unsigned long long* d_sums; rr_align_record* d_rec;
    RR_HIP(c, sc.room(d_xcorr ? 0 : chunk * A, d_curve));
    RR_HIP(c, sc.room(2 * (chunk + 1), d_sums));
    RR_HIP(c, sc.room(n, d_rec));
    for (size_t at = 0; at < n; at += kChunk) {
        const int m = (int)std::min(kChunk, n - at);
        const uint8_t* imgs = d_imgs_u8 + at * npx;
        long long* curve = d_xcorr ? reinterpret_cast<long long*>(d_xcorr) + at * A : d_curve;
        RR_HIP(c, hipMemsetAsync(curve, 0, (size_t)m * A * sizeof(long long), s));
        RR_HIP(c, hipMemsetAsync(d_sums, 0, 2 * ((size_t)m + 1) * sizeof(unsigned long long), s));
        launch_align_sums(imgs, d_ref_u8, g.n_cells, g.n_angles, cell_begin, cell_end, m, d_sums, s);
        launch_align_gram(imgs, d_ref_u8, g.n_cells, g.n_angles, cell_begin, cell_end, m, curve, s);
        launch_align_finish(curve, d_sums, m, g.n_angles, cell_begin, cell_end, d_rec + at, s);
    }
    std::vector<rr_align_record> rec(n);
    rc = records_back(c, rec.data(), d_rec, n * sizeof(rr_align_record), s); if (rc) return rc;
    const size_t n_win = (size_t)(cell_end - cell_begin) * A;
    for (size_t k = 0; k < n; k++) {
        rec[k].psnr = psnr_of(rec[k].sse, n_win);       // the host's log10, as rr_score_images_device
        out[k] = rec[k];
    }
    return 0;
}

int rr_align_images(rr_ctx* c, const uint8_t* imgs_u8, int n_images, const uint8_t* ref_u8, int cell_begin, int cell_end,
                    rr_align_record* out, int64_t* xcorr)
{
    int rc = check_align(c, "rr_align_images", imgs_u8, n_images, 65535, ref_u8, cell_begin, cell_end, out); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_images, A = (size_t)c->cfg.n_angles, npx = (size_t)c->cfg.n_cells * A;
    RR_STAGE(c, st);
    uint8_t* d_ref; int64_t* d_curve = nullptr;
    RR_HIP(c, st.up(ref_u8, npx, d_ref));
    if (xcorr) RR_HIP(c, st.room(std::min(n, kChunk) * A, d_curve));
    std::vector<rr_align_record> rec(n);
    rc = in_chunks(c, st, imgs_u8, n, npx, [&](const uint8_t* d_imgs, size_t at, size_t m) {
        const int rcc = rr_align_images_device(c, d_imgs, (int)m, d_ref, cell_begin, cell_end, rec.data() + at, d_curve, c->stream); if (rcc) return rcc;
        if (xcorr) RR_HIP(c, hipMemcpy(xcorr + at * A, d_curve, m * A * sizeof(int64_t), hipMemcpyDeviceToHost));
        return 0;
    }); if (rc) return rc;
    std::copy(rec.begin(), rec.end(), out);
    return 0;
}

int rr_simulate_batch_align(rr_ctx* c, const float* poses, int n_frames, const uint8_t* ref_img_u8, int cell_begin, int cell_end,
                            uint8_t* out_imgs_u8, rr_align_record* out, int64_t* xcorr)
{
    // refused before anything is simulated (the context stands in for the images: they are its own)
    int rc = check_align(c, "rr_simulate_batch_align", c, n_frames, RR_MAX_BATCH, ref_img_u8, cell_begin, cell_end, out); if (rc) return rc;
    rc = check_ready(c); if (rc) return rc;
    if (!poses) return fail(c, -3, "rr_simulate_batch_align: null poses");
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n = (size_t)n_frames, A = (size_t)c->cfg.n_angles;
    RR_STAGE(c, st);
    uint8_t *d_imgs, *d_ref; int64_t* d_curve = nullptr;
    RR_HIP(c, st.room(n * npx, d_imgs));
    RR_HIP(c, st.up(ref_img_u8, npx, d_ref));
    if (xcorr) RR_HIP(c, st.room(n * A, d_curve));
    rc = rr_simulate_batch_device(c, poses, n_frames, d_imgs, c->stream); if (rc) return rc;
    std::vector<rr_align_record> rec(n);
    rc = rr_align_images_device(c, d_imgs, n_frames, d_ref, cell_begin, cell_end, rec.data(), d_curve, c->stream); if (rc) return rc;
    st.out(out_imgs_u8, d_imgs, n * npx, false);
    st.out(xcorr, d_curve, n * A, false);
    rc = st.commit(frame_gate(c)); if (rc) return rc;
    std::copy(rec.begin(), rec.end(), out);
    return 0;
}

// ---- translation registration: the 2-D cross-correlation over a window of pixel shifts (rr_shift.hip) ----------------

int rr_shift_images_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n_images, const uint8_t* d_ref_u8, int height, int width, int max_shift,
                           rr_shift_record* out, int64_t* d_xcorr, uint64_t* d_sse, void* stream)
{
    int rc = check_shift(c, "rr_shift_images_device", d_imgs_u8, n_images, 65535, d_ref_u8, height, width, max_shift, out); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    const int H = height, W = width, S = max_shift, D = 2 * S + 1;
    const size_t npx = (size_t)H * W, n = (size_t)n_images, ND = (size_t)D * D, n_col = 2 * (size_t)D * W;
    const size_t chunk = std::min(n, kChunk);
    static_assert(sizeof(long long) == sizeof(int64_t) && sizeof(unsigned long long) == sizeof(uint64_t), "surface words");
    // one chunk's surface (when the caller gives no buffer) and sums, the reference's column and box sums, the records
    Scratch sc(c->scratch_of(s), s);
    long long* d_surf; unsigned long long *d_sums, *d_col, *d_box; rr_shift_record* d_rec;
    RR_HIP(c, sc.room(d_xcorr ? 0 : chunk * ND, d_surf));
    RR_HIP(c, sc.room(2 * chunk, d_sums));
    RR_HIP(c, sc.room(n_col, d_col));
    RR_HIP(c, sc.room(2 * ND, d_box));
    RR_HIP(c, sc.room(n, d_rec));
    launch_shift_box(d_ref_u8, H, W, S, d_col, d_box, s);      // once per call: every image meets the same reference
    for (size_t at = 0; at < n; at += kChunk) {
        const int m = (int)std::min(kChunk, n - at);
        const uint8_t* imgs = d_imgs_u8 + at * npx;
        long long* surf = d_xcorr ? reinterpret_cast<long long*>(d_xcorr) + at * ND : d_surf;
        unsigned long long* sse = d_sse ? reinterpret_cast<unsigned long long*>(d_sse) + at * ND : nullptr;
        RR_HIP(c, hipMemsetAsync(surf, 0, (size_t)m * ND * sizeof(long long), s));
        RR_HIP(c, hipMemsetAsync(d_sums, 0, 2 * (size_t)m * sizeof(unsigned long long), s));
        launch_shift_sums(imgs, H, W, S, m, d_sums, s);
        launch_shift_gram(imgs, d_ref_u8, H, W, S, m, surf, s);
        launch_shift_finish(surf, sse, d_sums, d_box, H, W, S, m, d_rec + at, s);
    }
    std::vector<rr_shift_record> rec(n);
    rc = records_back(c, rec.data(), d_rec, n * sizeof(rr_shift_record), s); if (rc) return rc;
    const size_t n_win = (size_t)(H - 2 * S) * (W - 2 * S);
    // the sub-pixel offset along one axis from the exact SSE before, at and after the best shift (each below 2^39)
    auto sub = [](uint64_t before, uint64_t at_best, uint64_t after) {
        if (before == UINT64_MAX || after == UINT64_MAX) return 0.0;
        const int64_t num = (int64_t)before - (int64_t)after, den = (int64_t)before - 2 * (int64_t)at_best + (int64_t)after;
        return den <= 0 ? 0.0 : 0.5 * (double)num / (double)den;
    };
    for (size_t k = 0; k < n; k++) {
        rr_shift_record& r = rec[k];
        r.psnr = psnr_of(r.sse, n_win);                 // the host's log10, as rr_score_images_device
        r.sub_dy = sub(r.sse_nb[0], r.sse, r.sse_nb[1]);
        r.sub_dx = sub(r.sse_nb[2], r.sse, r.sse_nb[3]);
        out[k] = r;
    }
    return 0;
}

int rr_shift_images(rr_ctx* c, const uint8_t* imgs_u8, int n_images, const uint8_t* ref_u8, int height, int width, int max_shift,
                    rr_shift_record* out, int64_t* xcorr, uint64_t* sse)
{
    int rc = check_shift(c, "rr_shift_images", imgs_u8, n_images, 65535, ref_u8, height, width, max_shift, out); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_images, npx = (size_t)height * width, D = 2 * (size_t)max_shift + 1, ND = D * D, chunk = std::min(n, kChunk);
    RR_STAGE(c, st);
    uint8_t* d_ref; int64_t* d_xcorr = nullptr; uint64_t* d_sse = nullptr;
    RR_HIP(c, st.up(ref_u8, npx, d_ref));
    if (xcorr) RR_HIP(c, st.room(chunk * ND, d_xcorr));
    if (sse) RR_HIP(c, st.room(chunk * ND, d_sse));
    std::vector<rr_shift_record> rec(n);
    rc = in_chunks(c, st, imgs_u8, n, npx, [&](const uint8_t* d_imgs, size_t at, size_t m) {
        const int rcc = rr_shift_images_device(c, d_imgs, (int)m, d_ref, height, width, max_shift, rec.data() + at, d_xcorr, d_sse, c->stream);
        if (rcc) return rcc;
        if (xcorr) RR_HIP(c, hipMemcpy(xcorr + at * ND, d_xcorr, m * ND * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (sse) RR_HIP(c, hipMemcpy(sse + at * ND, d_sse, m * ND * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return 0;
    }); if (rc) return rc;
    std::copy(rec.begin(), rec.end(), out);
    return 0;
}

int rr_simulate_batch_shift(rr_ctx* c, const float* poses, int n_frames, const uint8_t* ref_polar_u8, const rr_cartesian_config* cfg,
                            int max_shift, uint8_t* out_cart_u8, rr_shift_record* out, int64_t* xcorr)
{
    // refused before anything is simulated (the context stands in for the images: they are its own)
    int rc = check_cartesian(c, "rr_simulate_batch_shift", ref_polar_u8, 1, cfg, out); if (rc) return rc;
    rc = check_shift(c, "rr_simulate_batch_shift", c, n_frames, RR_MAX_BATCH, ref_polar_u8, cfg->width, cfg->width, max_shift, out); if (rc) return rc;
    rc = check_ready(c); if (rc) return rc;
    if (!poses) return fail(c, -3, "rr_simulate_batch_shift: null poses");
    RR_HIP(c, hipSetDevice(c->device));
    const rr_config& g = c->cfg;
    const size_t npx = (size_t)g.n_cells * g.n_angles, n = (size_t)n_frames, ncart = (size_t)cfg->width * cfg->width;
    const size_t D = 2 * (size_t)max_shift + 1, ND = D * D;
    RR_STAGE(c, st);
    uint8_t *d_imgs, *d_ref, *d_cart, *d_ref_cart; int64_t* d_xcorr = nullptr;
    RR_HIP(c, st.room(n * npx, d_imgs));
    RR_HIP(c, st.up(ref_polar_u8, npx, d_ref));
    RR_HIP(c, st.room(n * ncart, d_cart));
    RR_HIP(c, st.room(ncart, d_ref_cart));
    if (xcorr) RR_HIP(c, st.room(n * ND, d_xcorr));
    rc = rr_simulate_batch_device(c, poses, n_frames, d_imgs, c->stream); if (rc) return rc;
    const PolarGrid G = polar_grid(g);
    launch_cartesian(d_imgs, n_frames, *cfg, G, d_cart, c->stream);
    launch_cartesian(d_ref, 1, *cfg, G, d_ref_cart, c->stream);
    std::vector<rr_shift_record> rec(n);
    rc = rr_shift_images_device(c, d_cart, n_frames, d_ref_cart, cfg->width, cfg->width, max_shift, rec.data(), d_xcorr, nullptr, c->stream);
    if (rc) return rc;
    st.out(out_cart_u8, d_cart, n * ncart, false);
    st.out(xcorr, d_xcorr, n * ND, false);
    rc = st.commit(frame_gate(c)); if (rc) return rc;
    std::copy(rec.begin(), rec.end(), out);
    return 0;
}

// ---- place recognition: ring/sector descriptors and their exact matching (rr_place.hip) ------------------------------

int rr_describe_images_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n, const rr_place_config* cfg, uint8_t* d_desc, void* stream)
{
    int rc = check_describe(c, "rr_describe_images_device", d_imgs_u8, n, 65535, cfg, d_desc); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_place_describe(d_imgs_u8, n, c->cfg.n_cells, c->cfg.n_angles, *cfg, d_desc, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_describe_images(rr_ctx* c, const uint8_t* imgs_u8, int n, const rr_place_config* cfg, uint8_t* desc)
{
    int rc = check_describe(c, "rr_describe_images", imgs_u8, n, 65535, cfg, desc); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, K = (size_t)cfg->n_rings * cfg->n_sectors, total = (size_t)n;
    RR_STAGE(c, st);
    uint8_t* d_desc;
    RR_HIP(c, st.room(std::min(total, kChunk) * K, d_desc));
    std::vector<uint8_t> all(total * K);                    // the caller's buffer is written once every chunk has succeeded
    rc = in_chunks(c, st, imgs_u8, total, npx, [&](const uint8_t* d_imgs, size_t at, size_t m) {
        const int rcc = rr_describe_images_device(c, d_imgs, (int)m, cfg, d_desc, c->stream); if (rcc) return rcc;
        RR_HIP(c, hipMemcpyAsync(all.data() + at * K, d_desc, m * K, hipMemcpyDeviceToHost, c->stream));
        RR_HIP(c, hipStreamSynchronize(c->stream));         // the rooms are free again
        return 0;
    }); if (rc) return rc;
    std::copy(all.begin(), all.end(), desc);
    return 0;
}

int rr_simulate_batch_describe(rr_ctx* c, const float* poses, int n_frames, const rr_place_config* cfg, uint8_t* out_desc)
{
    // refused before anything is simulated (the context stands in for the images: they are its own)
    int rc = check_describe(c, "rr_simulate_batch_describe", c, n_frames, RR_MAX_BATCH, cfg, out_desc); if (rc) return rc;
    rc = check_ready(c); if (rc) return rc;
    if (!poses) return fail(c, -3, "rr_simulate_batch_describe: null poses");
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n = (size_t)n_frames, K = (size_t)cfg->n_rings * cfg->n_sectors;
    RR_STAGE(c, st);
    uint8_t *d_imgs, *d_desc;
    RR_HIP(c, st.room(n * npx, d_imgs));
    RR_HIP(c, st.hold(out_desc, n * K, d_desc));
    rc = rr_simulate_batch_device(c, poses, n_frames, d_imgs, c->stream); if (rc) return rc;
    rc = rr_describe_images_device(c, d_imgs, n_frames, cfg, d_desc, c->stream); if (rc) return rc;
    return st.commit(frame_gate(c));
}

int rr_match_descriptors_device(rr_ctx* c, const uint8_t* d_query, int n_query, const uint8_t* d_db, int n_db, int n_rings, int n_sectors, int top_k,
                                rr_place_match* out, uint32_t* d_sse, uint16_t* d_shift, void* stream)
{
    int rc = check_match(c, "rr_match_descriptors_device", d_query, n_query, d_db, n_db, n_rings, n_sectors, top_k, out, d_sse, d_shift); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    const size_t nq = (size_t)n_query, n = (size_t)n_db, k = (size_t)top_k, K = (size_t)n_rings * n_sectors;
    // the database in chunks of at most 2^22 (query, candidate) pairs, whole tiles of 32 candidates: 64 MB of keys and aux words
    const size_t chunk = std::min(n, std::max<size_t>(32, ((size_t)1 << 22) / nq / 32 * 32));
    const size_t n_rolls = nq * n_sectors * (size_t)place_kpad(n_rings, n_sectors), n_part = nq * place_slices(chunk) * k, n_win = nq * k;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "key words");
    // the rolled queries and their sums, one database chunk's keys and aux words, the slices' winners, the winners so far twice over, the records
    Scratch sc(c->scratch_of(s), s);
    uint8_t* d_rolls; uint32_t* d_qsums; unsigned long long *d_keys, *d_aux, *d_part, *d_win; rr_place_match* d_rec;
    RR_HIP(c, sc.room(n_rolls, d_rolls));
    RR_HIP(c, sc.room(2 * nq, d_qsums));
    RR_HIP(c, sc.room(nq * chunk, d_keys));
    RR_HIP(c, sc.room(nq * chunk, d_aux));
    RR_HIP(c, sc.room(n_part, d_part));
    RR_HIP(c, sc.room(4 * n_win, d_win));
    RR_HIP(c, sc.room(n_win, d_rec));
    launch_place_rolls(d_query, n_query, n_rings, n_sectors, d_rolls, d_qsums, s);
    // the winners so far, [2][keys | aux][n_query][top_k]: a chunk reads one half and writes the other.  No winner yet: every key ~0
    unsigned long long* half[2] = { d_win, d_win + 2 * n_win };
    RR_HIP(c, hipMemsetAsync(half[0], 0xFF, n_win * sizeof(unsigned long long), s));
    int cur = 0;
    for (size_t at = 0; at < n; at += chunk, cur ^= 1) {
        const size_t m = std::min(chunk, n - at);
        launch_place_match(d_rolls, d_qsums, n_query, d_db + at * K, m, at, n_rings, n_sectors, d_keys, d_aux, d_sse, d_shift, n, s);
        launch_place_topk(d_keys, d_aux, n_query, m, at, top_k, d_part, half[cur], half[cur] + n_win, half[cur ^ 1], half[cur ^ 1] + n_win, s);
    }
    launch_place_finish(half[cur], half[cur] + n_win, d_qsums, n_query, top_k, n_rings, n_sectors, d_rec, s);
    std::vector<rr_place_match> rec(n_win);
    rc = records_back(c, rec.data(), d_rec, n_win * sizeof(rr_place_match), s); if (rc) return rc;
    for (size_t e = 0; e < n_win; e++) {
        rec[e].psnr = psnr_of(rec[e].sse, K);           // the host's log10, as rr_score_images_device
        out[e] = rec[e];
    }
    return 0;
}

int rr_match_descriptors(rr_ctx* c, const uint8_t* query, int n_query, const uint8_t* db, int n_db, int n_rings, int n_sectors, int top_k,
                         rr_place_match* out, uint32_t* sse, uint16_t* shift)
{
    int rc = check_match(c, "rr_match_descriptors", query, n_query, db, n_db, n_rings, n_sectors, top_k, out, sse, shift); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t nq = (size_t)n_query, n = (size_t)n_db, k = (size_t)top_k, K = (size_t)n_rings * n_sectors;
    // the database goes up 16 MiB at a time; the chunks' winners are merged here by the same key
    const size_t chunk = std::min(n, std::max<size_t>(k, ((size_t)16 << 20) / K));
    RR_STAGE(c, st);
    uint8_t *d_query, *d_db; uint32_t* d_sse = nullptr; uint16_t* d_shift = nullptr;
    RR_HIP(c, st.up(query, nq * K, d_query));
    RR_HIP(c, st.room(chunk * K, d_db));
    if (sse) RR_HIP(c, st.room(nq * chunk, d_sse));
    if (shift) RR_HIP(c, st.room(nq * chunk, d_shift));
    auto before = [](const rr_place_match& a, const rr_place_match& b) { return a.sse != b.sse ? a.sse < b.sse : a.index < b.index; };
    std::vector<std::vector<rr_place_match>> best(nq);
    std::vector<rr_place_match> rec(nq * k);
    std::vector<uint32_t> sse_all(sse ? nq * n : 0);
    std::vector<uint16_t> shift_all(shift ? nq * n : 0);
    for (size_t at = 0; at < n; at += chunk) {
        const size_t m = std::min(chunk, n - at), km = std::min(k, m);
        RR_HIP(c, st.again(d_db, db + at * K, m * K));
        rc = rr_match_descriptors_device(c, d_query, n_query, d_db, (int)m, n_rings, n_sectors, (int)km, rec.data(), d_sse, d_shift, c->stream); if (rc) return rc;
        for (size_t q = 0; q < nq; q++) {
            for (size_t j = 0; j < km; j++) { rr_place_match r = rec[q * km + j]; r.index += (uint32_t)at; best[q].push_back(r); }
            std::sort(best[q].begin(), best[q].end(), before);
            if (best[q].size() > k) best[q].resize(k);
            if (sse) RR_HIP(c, hipMemcpy(sse_all.data() + q * n + at, d_sse + q * m, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
            if (shift) RR_HIP(c, hipMemcpy(shift_all.data() + q * n + at, d_shift + q * m, m * sizeof(uint16_t), hipMemcpyDeviceToHost));
        }
    }
    for (size_t q = 0; q < nq; q++) std::copy(best[q].begin(), best[q].end(), out + q * k);
    if (sse) std::copy(sse_all.begin(), sse_all.end(), sse);
    if (shift) std::copy(shift_all.begin(), shift_all.end(), shift);
    return 0;
}

// ---- point clouds and Cartesian images (rr_detect.hip) ---------------------------------------------------------------
void rr_default_detect_config(rr_detect_config* cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->method = 0; cfg->guard_cells = 2; cfg->train_cells = 16; cfg->k = 12;
    cfg->min_intensity = 1; cfg->min_bin = 0; cfg->cfar_scale = 3.0f;
}

int rr_detect_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n_frames, const rr_detect_config* cfg, rr_radar_point* d_points,
                     int max_points, uint32_t* d_offsets, void* stream)
{
    int rc = check_detect(c, "rr_detect_device", d_imgs_u8, n_frames, cfg, d_points, max_points, d_offsets); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_detect(d_imgs_u8, n_frames, *cfg, polar_grid(c->cfg), max_points > 0 ? d_points : nullptr, max_points, d_offsets, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_detect(rr_ctx* c, const uint8_t* imgs_u8, int n_frames, const rr_detect_config* cfg, rr_radar_point* points,
              int max_points, uint32_t* offsets)
{
    int rc = check_detect(c, "rr_detect", imgs_u8, n_frames, cfg, points, max_points, offsets); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n_offs = (size_t)n_frames * (c->cfg.n_angles + 1), n_pts = (size_t)n_frames * (size_t)max_points;
    RR_STAGE(c, st);
    uint8_t* d_imgs; uint32_t* d_offs; rr_radar_point* d_points = nullptr;
    RR_HIP(c, st.up(imgs_u8, (size_t)n_frames * npx, d_imgs));
    RR_HIP(c, st.room(n_offs, d_offs));
    if (n_pts) RR_HIP(c, st.room(n_pts, d_points));
    rc = rr_detect_device(c, d_imgs, n_frames, cfg, d_points, max_points, d_offs, c->stream); if (rc) return rc;
    st.out(offsets, d_offs, n_offs, false);
    if (n_pts) st.out(points, d_points, n_pts, false);
    return st.commit();
}

// ---- windowed CFAR (rr_window.hip) -------------------------------------------------------------------------------------
void rr_default_window_detect_config(rr_window_detect_config* cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->method = 3; cfg->guard_range = 2; cfg->train_range = 16; cfg->guard_azimuth = 1; cfg->train_azimuth = 2;
    cfg->rank_permille = 750; cfg->min_intensity = 1; cfg->min_bin = 0; cfg->scale = 3.0f;
}

// what is wrong with a window config for images of n_cells x n_angles, or null
static const char* window_config_error(const rr_window_detect_config* d, int n_cells, int n_angles)
{
    if (!d) return "null config";
    if (d->method < 0 || d->method > 3) return "method must be 0 (CA), 1 (GO), 2 (SO) or 3 (OS)";
    if (d->guard_range < 0 || d->guard_range > 1024) return "guard_range must be 0..1024";
    if (d->train_range < 0 || d->train_range > 1024) return "train_range must be 0..1024";
    if (d->guard_azimuth < 0 || d->guard_azimuth > 32) return "guard_azimuth must be 0..32";
    if (d->train_azimuth < 0 || d->train_azimuth > 32) return "train_azimuth must be 0..32";
    if (d->rank_permille < 1 || d->rank_permille > 1000) return "rank_permille must be 1..1000";
    if (d->min_intensity < 0 || d->min_intensity > 255) return "min_intensity must be 0..255";
    if (d->min_bin < 0 || d->min_bin >= n_cells) return "min_bin must be 0..n_cells-1";
    if (!(std::isfinite(d->scale) && d->scale >= 0.0f)) return "scale must be finite and >= 0";
    if (d->reserved_[0] || d->reserved_[1] || d->reserved_[2]) return "reserved_ must be 0";
    if (d->train_range + d->train_azimuth == 0) return "no training cells: train_range + train_azimuth is 0";
    const int wc = 2 * (d->guard_azimuth + d->train_azimuth) + 1, wr = 2 * (d->guard_range + d->train_range) + 1;
    if (wc > n_angles) return "the column window 2 (guard_azimuth + train_azimuth) + 1 exceeds n_angles";
    if ((long long)wr * wc > 65535) return "a window of more than 65,535 cells";
    if ((d->method == 1 || d->method == 2) && d->train_range == 0) return "GO / SO need train_range >= 1";
    return nullptr;
}

static int check_detect_window(rr_ctx* c, const char* who, const void* imgs, int n_frames, const rr_window_detect_config* d, const void* points,
                               int max_points, const void* offsets)
{
    const std::string w(who);
    int rc = check_images(c, w, imgs != nullptr, "images", "n_frames", n_frames, 65535); if (rc) return rc;
    if (!offsets) return fail(c, -3, w + ": null offsets");
    if (max_points < 0) return fail(c, -3, w + ": max_points must be >= 0");
    if (max_points > 0 && !points) return fail(c, -3, w + ": null points with max_points > 0");
    if (const char* e = window_config_error(d, c->cfg.n_cells, c->cfg.n_angles)) return fail(c, -3, w + ": " + e);
    return 0;
}

int rr_detect_window_tile_sizes(const rr_window_detect_config* cfg, int n_cells, int n_angles, int out[4])
{
    if (!out || n_cells < 1 || n_angles < 1 || window_config_error(cfg, n_cells, n_angles)) return -3;
    return window_tile_sizes(*cfg, n_cells, n_angles, out) ? 0 : -3;
}

int rr_detect_window_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n_frames, const rr_window_detect_config* cfg, rr_radar_point* d_points,
                            int max_points, uint32_t* d_offsets, uint8_t* d_mask, void* stream)
{
    int rc = check_detect_window(c, "rr_detect_window_device", d_imgs_u8, n_frames, cfg, d_points, max_points, d_offsets); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, launch_detect_window(d_imgs_u8, n_frames, *cfg, polar_grid(c->cfg), max_points > 0 ? d_points : nullptr, max_points, d_offsets, d_mask,
                                   stream_of(c, stream)));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_detect_window(rr_ctx* c, const uint8_t* imgs_u8, int n_frames, const rr_window_detect_config* cfg, rr_radar_point* points,
                     int max_points, uint32_t* offsets, uint8_t* mask)
{
    int rc = check_detect_window(c, "rr_detect_window", imgs_u8, n_frames, cfg, points, max_points, offsets); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n_offs = (size_t)n_frames * (c->cfg.n_angles + 1), n_pts = (size_t)n_frames * (size_t)max_points;
    RR_STAGE(c, st);
    uint8_t *d_imgs, *d_mask = nullptr; uint32_t* d_offs; rr_radar_point* d_points = nullptr;
    RR_HIP(c, st.up(imgs_u8, (size_t)n_frames * npx, d_imgs));
    RR_HIP(c, st.room(n_offs, d_offs));
    if (n_pts) RR_HIP(c, st.room(n_pts, d_points));
    if (mask) RR_HIP(c, st.room((size_t)n_frames * npx, d_mask));
    rc = rr_detect_window_device(c, d_imgs, n_frames, cfg, d_points, max_points, d_offs, d_mask, c->stream); if (rc) return rc;
    st.out(offsets, d_offs, n_offs, false);
    if (n_pts) st.out(points, d_points, n_pts, false);
    if (mask) st.out(mask, d_mask, (size_t)n_frames * npx, false);
    return st.commit();
}

int rr_polar_to_cartesian_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n_frames, const rr_cartesian_config* cfg,
                                 uint8_t* d_cart_u8, void* stream)
{
    int rc = check_cartesian(c, "rr_polar_to_cartesian_device", d_imgs_u8, n_frames, cfg, d_cart_u8); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_cartesian(d_imgs_u8, n_frames, *cfg, polar_grid(c->cfg), d_cart_u8, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_polar_to_cartesian(rr_ctx* c, const uint8_t* imgs_u8, int n_frames, const rr_cartesian_config* cfg, uint8_t* cart_u8)
{
    int rc = check_cartesian(c, "rr_polar_to_cartesian", imgs_u8, n_frames, cfg, cart_u8); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n_out = (size_t)n_frames * cfg->width * cfg->width;
    RR_STAGE(c, st);
    uint8_t *d_imgs, *d_cart;
    RR_HIP(c, st.up(imgs_u8, (size_t)n_frames * npx, d_imgs));
    RR_HIP(c, st.room(n_out, d_cart));
    rc = rr_polar_to_cartesian_device(c, d_imgs, n_frames, cfg, d_cart, c->stream); if (rc) return rc;
    st.out(cart_u8, d_cart, n_out, false);
    return st.commit();
}

// ---- sweep compensation (rr_deskew.hip) -------------------------------------------------------------------------------
int rr_sweep_table_device(rr_ctx* c, const float* d_az_poses, const float* d_ref_poses, const float* d_sensor_vel, float gain, int n_frames,
                          rr_sweep_rec* d_table, void* stream)
{
    int rc = check_sweep_table(c, "rr_sweep_table_device", d_az_poses, d_ref_poses, gain, n_frames, d_table, true); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_sweep_table(d_az_poses, d_ref_poses, d_sensor_vel, gain, n_frames, polar_grid(c->cfg), d_table, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_sweep_table(rr_ctx* c, const float* az_poses, const float* ref_poses, const float* sensor_vel, float gain, int n_frames, rr_sweep_rec* table)
{
    const std::string w("rr_sweep_table");
    int rc = check_sweep_table(c, w.c_str(), az_poses, ref_poses, gain, n_frames, table, false); if (rc) return rc;
    const size_t n = (size_t)n_frames, A = (size_t)c->cfg.n_angles, n_az = n * A * 7, n_ref = n * 7, n_vel = sensor_vel ? n * 3 : 0;
    auto finite = [](const float* p, size_t m) { for (size_t i = 0; i < m; i++) if (!std::isfinite(p[i])) return false; return true; };
    auto unit = [](const float* p, size_t m) {
        for (size_t i = 0; i < m; i++) {
            const float* q = p + 7 * i;
            const double nn = (double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2] + (double)q[3] * q[3];
            if (!(std::fabs(nn - 1.0) <= 1e-3)) return false;
        }
        return true;
    };
    if (!finite(az_poses, n_az) || !finite(ref_poses, n_ref) || !finite(sensor_vel, n_vel)) return fail(c, -3, w + ": a non-finite pose or velocity");
    if (!unit(az_poses, n * A) || !unit(ref_poses, n)) return fail(c, -3, w + ": a quaternion whose squared norm is off 1 by more than 1e-3");
    RR_HIP(c, hipSetDevice(c->device));
    RR_STAGE(c, st);
    float *d_az, *d_ref, *d_vel; rr_sweep_rec* d_table;
    RR_HIP(c, st.up(az_poses, n_az, d_az));
    RR_HIP(c, st.up(ref_poses, n_ref, d_ref));
    RR_HIP(c, st.up(sensor_vel, n_vel, d_vel));
    RR_HIP(c, st.hold(table, n * A, d_table));
    rc = rr_sweep_table_device(c, d_az, d_ref, d_vel, gain, n_frames, d_table, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_compensate_points_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points,
                                const rr_sweep_rec* d_table, rr_radar_point* d_out, void* stream)
{
    int rc = check_compensate(c, "rr_compensate_points_device", d_points, d_offsets, n_frames, max_points, d_table, d_out, true); if (rc) return rc;
    if (max_points == 0) return 0;
    RR_HIP(c, hipSetDevice(c->device));
    launch_compensate_points(d_points, d_offsets, n_frames, max_points, d_table, d_out, polar_grid(c->cfg), stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_compensate_points(rr_ctx* c, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const rr_sweep_rec* table,
                         rr_radar_point* out)
{
    int rc = check_compensate(c, "rr_compensate_points", points, offsets, n_frames, max_points, table, out, false); if (rc) return rc;
    if (max_points == 0) return 0;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_frames, A = (size_t)c->cfg.n_angles, mp = (size_t)max_points;
    RR_STAGE(c, st);
    std::vector<uint32_t> totals; rr_radar_point* d_points; uint32_t* d_offs; rr_sweep_rec* d_table;
    rc = up_points(c, st, points, offsets, n, mp, totals, d_points, d_offs); if (rc) return rc;
    RR_HIP(c, st.up(table, n * A, d_table));
    rc = rr_compensate_points_device(c, d_points, d_offs, n_frames, max_points, d_table, d_points, c->stream); if (rc) return rc;      // in place
    st.out_rows(out, d_points, n, mp, mp, totals.data());
    return st.commit();
}

int rr_polar_to_cartesian_sweep_device(rr_ctx* c, const uint8_t* d_imgs_u8, int n_frames, const rr_cartesian_config* cfg, const rr_sweep_rec* d_table,
                                       int iterations, uint8_t* d_cart_u8, void* stream)
{
    int rc = check_cartesian_sweep(c, "rr_polar_to_cartesian_sweep_device", d_imgs_u8, n_frames, cfg, d_table, iterations, d_cart_u8, true); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_cartesian_sweep(d_imgs_u8, n_frames, *cfg, polar_grid(c->cfg), d_table, iterations, d_cart_u8, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_polar_to_cartesian_sweep(rr_ctx* c, const uint8_t* imgs_u8, int n_frames, const rr_cartesian_config* cfg, const rr_sweep_rec* table, int iterations,
                                uint8_t* cart_u8)
{
    int rc = check_cartesian_sweep(c, "rr_polar_to_cartesian_sweep", imgs_u8, n_frames, cfg, table, iterations, cart_u8, false);
    if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_frames, A = (size_t)c->cfg.n_angles, npx = (size_t)c->cfg.n_cells * A, n_out = n * cfg->width * cfg->width;
    RR_STAGE(c, st);
    uint8_t *d_imgs, *d_cart; rr_sweep_rec* d_table;
    RR_HIP(c, st.up(imgs_u8, n * npx, d_imgs));
    RR_HIP(c, st.up(table, n * A, d_table));
    RR_HIP(c, st.room(n_out, d_cart));
    rc = rr_polar_to_cartesian_sweep_device(c, d_imgs, n_frames, cfg, d_table, iterations, d_cart, c->stream); if (rc) return rc;
    st.out(cart_u8, d_cart, n_out, false);
    return st.commit();
}

// ---- scan matching (rr_icp.hip) ----------------------------------------------------------------------------------------
void rr_icp_tile_sizes(int* source_tile, int* target_tile) { icp_tile_sizes(source_tile, target_tile); }

int rr_register_points_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points,
                              const rr_radar_point* d_tgt_points, const uint32_t* d_tgt_count, int max_tgt, const double* d_init, float gate,
                              int iterations, rr_icp_rec* d_recs, uint32_t* d_corr, void* stream)
{
    return register_device<PointMatch>(c, "rr_register_points_device", d_points, d_offsets, n_frames, max_points, d_tgt_points, d_tgt_count, max_tgt, d_init,
                                       gate, iterations, d_recs, d_corr, stream);
}

int rr_register_points(rr_ctx* c, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const rr_radar_point* tgt_points,
                       uint32_t tgt_count, int max_tgt, const double* init, float gate, int iterations, rr_icp_rec* recs, uint32_t* corr)
{
    return register_host<PointMatch>(c, "rr_register_points", points, offsets, n_frames, max_points, tgt_points, tgt_count, max_tgt, init, gate, iterations,
                                     recs, corr);
}

// (rr_surfels.hip makes the target of this one)
int rr_register_surfels_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points,
                               const rr_surfel* d_tgt_surfels, const uint32_t* d_tgt_count, int max_tgt, const double* d_init, float gate,
                               int iterations, rr_icp_rec* d_recs, uint32_t* d_corr, void* stream)
{
    return register_device<LineMatch>(c, "rr_register_surfels_device", d_points, d_offsets, n_frames, max_points, d_tgt_surfels, d_tgt_count, max_tgt, d_init,
                                      gate, iterations, d_recs, d_corr, stream);
}

int rr_register_surfels(rr_ctx* c, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const rr_surfel* tgt_surfels,
                        uint32_t tgt_count, int max_tgt, const double* init, float gate, int iterations, rr_icp_rec* recs, uint32_t* corr)
{
    return register_host<LineMatch>(c, "rr_register_surfels", points, offsets, n_frames, max_points, tgt_surfels, tgt_count, max_tgt, init, gate, iterations,
                                    recs, corr);
}

// ---- likelihood field (rr_field.hip) ------------------------------------------------------------------------------------
void rr_field_tile_sizes(int* points_tile, int* hyps_per_group, int* row_tile) { field_tile_sizes(points_tile, hyps_per_group, row_tile); }

int rr_rasterize_points_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points,
                               const double* d_states, const rr_field_config* cfg, uint8_t* d_occ_u8, void* stream)
{
    int rc = check_rasterize(c, "rr_rasterize_points_device", d_points, d_offsets, n_frames, max_points, d_states, cfg, d_occ_u8); if (rc) return rc;
    if (max_points == 0) return 0;
    RR_HIP(c, hipSetDevice(c->device));
    launch_field_raster(d_points, d_offsets, n_frames, c->cfg.n_angles, max_points, d_states, *cfg, d_occ_u8, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_rasterize_points(rr_ctx* c, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const double* states,
                        const rr_field_config* cfg, uint8_t* occ_u8)
{
    int rc = check_rasterize(c, "rr_rasterize_points", points, offsets, n_frames, max_points, nullptr, cfg, occ_u8); if (rc) return rc;
    if (max_points == 0) return 0;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_frames, cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    std::vector<uint32_t> totals; rr_radar_point* d_points; uint32_t* d_offs; double* d_states; uint8_t* d_occ;
    rc = up_points(c, st, points, offsets, n, (size_t)max_points, totals, d_points, d_offs); if (rc) return rc;
    RR_HIP(c, st.up(states, n * 4, d_states));
    RR_HIP(c, st.up(occ_u8, cells, d_occ));      // the call accumulates
    rc = rr_rasterize_points_device(c, d_points, d_offs, n_frames, max_points, d_states, cfg, d_occ, c->stream); if (rc) return rc;
    st.out(occ_u8, d_occ, cells);
    return st.commit();
}

int rr_distance_field_device(rr_ctx* c, const uint8_t* d_occ_u8, int threshold, const rr_field_config* cfg, uint16_t* d_field_u16, void* stream)
{
    int rc = check_distance_field(c, "rr_distance_field_device", d_occ_u8, threshold, cfg, d_field_u16); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_distance_field(d_occ_u8, threshold, *cfg, d_field_u16, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_distance_field(rr_ctx* c, const uint8_t* occ_u8, int threshold, const rr_field_config* cfg, uint16_t* field_u16)
{
    int rc = check_distance_field(c, "rr_distance_field", occ_u8, threshold, cfg, field_u16); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    uint8_t* d_occ; uint16_t* d_field;
    RR_HIP(c, st.up(occ_u8, cells, d_occ));
    RR_HIP(c, st.hold(field_u16, cells, d_field));
    rc = rr_distance_field_device(c, d_occ, threshold, cfg, d_field, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_score_poses_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_count, int max_points, const float* d_states, int n_hyp,
                          const uint16_t* d_field_u16, const rr_field_config* cfg, rr_field_rec* d_recs, void* stream)
{
    int rc = check_score_poses(c, "rr_score_poses_device", d_points, d_count != nullptr, max_points, d_states, n_hyp, d_field_u16, cfg, d_recs);
    if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_field_score(d_points, d_count, max_points, d_states, n_hyp, d_field_u16, *cfg, d_recs, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_score_poses(rr_ctx* c, const rr_radar_point* points, uint32_t count, int max_points, const float* states, int n_hyp, const uint16_t* field_u16,
                   const rr_field_config* cfg, rr_field_rec* recs)
{
    int rc = check_score_poses(c, "rr_score_poses", points, true, max_points, states, n_hyp, field_u16, cfg, recs); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_hyp, cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    rr_radar_point* d_points; uint32_t* d_count; float* d_states; uint16_t* d_field; rr_field_rec* d_recs;
    RR_HIP(c, st.up_rows(points, 1, (size_t)max_points, &count, d_points));
    RR_HIP(c, st.up(&count, 1, d_count));
    RR_HIP(c, st.up(states, n * 4, d_states));
    RR_HIP(c, st.up(field_u16, cells, d_field));
    RR_HIP(c, st.hold(recs, n, d_recs));
    RR_HIP(c, hipStreamSynchronize(c->stream));        // (count is this call's own variable)
    rc = rr_score_poses_device(c, d_points, d_count, max_points, d_states, n_hyp, d_field, cfg, d_recs, c->stream); if (rc) return rc;
    return st.commit();
}

// ---- occupancy mapping (rr_occupancy.hip) ---------------------------------------------------------------------------------
void rr_occupancy_tile_sizes(int* cells_per_group, int* cells_per_thread, int* scan_chunk)
{
    occupancy_tile_sizes(cells_per_group, cells_per_thread, scan_chunk);
}

int rr_occupancy_update_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points,
                               const double* d_states, const rr_field_config* cfg, const rr_occupancy_config* occ_cfg, float* d_profile,
                               int32_t* d_evidence_i32, void* stream)
{
    int rc = check_occupancy_update(c, "rr_occupancy_update_device", d_points, d_offsets, n_frames, max_points, d_states, cfg, occ_cfg,
                                    d_profile != nullptr, d_profile, d_evidence_i32); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_occupancy_update(d_points, d_offsets, n_frames, max_points, d_states, *cfg, *occ_cfg, polar_grid(c->cfg), d_profile, d_evidence_i32,
                            stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_occupancy_update(rr_ctx* c, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const double* states,
                        const rr_field_config* cfg, const rr_occupancy_config* occ_cfg, int32_t* evidence_i32)
{
    int rc = check_occupancy_update(c, "rr_occupancy_update", points, offsets, n_frames, max_points, nullptr, cfg, occ_cfg, true, nullptr,
                                    evidence_i32); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_frames, cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    std::vector<uint32_t> totals; rr_radar_point* d_points; uint32_t* d_offs; double* d_states; float* d_profile; int32_t* d_ev;
    rc = up_points(c, st, points, offsets, n, (size_t)max_points, totals, d_points, d_offs); if (rc) return rc;
    RR_HIP(c, st.up(states, n * 4, d_states));
    RR_HIP(c, st.room(n * (size_t)c->cfg.n_angles, d_profile));
    RR_HIP(c, st.up(evidence_i32, cells, d_ev));      // the call accumulates
    rc = rr_occupancy_update_device(c, d_points, d_offs, n_frames, max_points, d_states, cfg, occ_cfg, d_profile, d_ev, c->stream); if (rc) return rc;
    st.out(evidence_i32, d_ev, cells);
    return st.commit();
}

int rr_occupancy_map_device(rr_ctx* c, const int32_t* d_evidence_i32, const rr_field_config* cfg, uint8_t* d_occ_u8, void* stream)
{
    int rc = check_occupancy_map(c, "rr_occupancy_map_device", d_evidence_i32, cfg, d_occ_u8); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_occupancy_map(d_evidence_i32, *cfg, d_occ_u8, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_occupancy_map(rr_ctx* c, const int32_t* evidence_i32, const rr_field_config* cfg, uint8_t* occ_u8)
{
    int rc = check_occupancy_map(c, "rr_occupancy_map", evidence_i32, cfg, occ_u8); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    int32_t* d_ev; uint8_t* d_occ;
    RR_HIP(c, st.up(evidence_i32, cells, d_ev));
    RR_HIP(c, st.hold(occ_u8, cells, d_occ));
    rc = rr_occupancy_map_device(c, d_ev, cfg, d_occ, c->stream); if (rc) return rc;
    return st.commit();
}

// ---- particle filter step (rr_filter.hip) -----------------------------------------------------------------------------------
void rr_filter_tile_sizes(int* scan_tile, int* draws_per_group, int* search_tile) { filter_tile_sizes(scan_tile, draws_per_group, search_tile); }

int rr_filter_resample_device(rr_ctx* c, const rr_field_rec* d_recs, int n, const uint16_t* d_table, int n_out, const rr_filter_config* cfg,
                              uint64_t* d_cum, uint32_t* d_ancestors, rr_filter_summary* d_summary, void* stream)
{
    int rc = check_filter_resample(c, "rr_filter_resample_device", d_recs, n, d_table, n_out, cfg, d_cum, d_ancestors, d_summary); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_filter_resample(d_recs, n, d_table, n_out, *cfg, d_cum, d_ancestors, d_summary, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_filter_resample(rr_ctx* c, const rr_field_rec* recs, int n, const uint16_t* table, int n_out, const rr_filter_config* cfg, uint64_t* cum,
                       uint32_t* ancestors, rr_filter_summary* summary)
{
    int rc = check_filter_resample(c, "rr_filter_resample", recs, n, table, n_out, cfg, cum, ancestors, summary); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    RR_STAGE(c, st);
    rr_field_rec* d_recs; uint16_t* d_table; uint64_t* d_cum; uint32_t* d_anc; rr_filter_summary* d_sum;
    RR_HIP(c, st.up(recs, (size_t)n, d_recs));
    RR_HIP(c, st.up(table, (size_t)cfg->n_table, d_table));
    RR_HIP(c, st.hold(cum, (size_t)n, d_cum));
    RR_HIP(c, st.hold(ancestors, (size_t)n_out, d_anc));
    RR_HIP(c, st.hold(summary, 1, d_sum));
    rc = rr_filter_resample_device(c, d_recs, n, d_table, n_out, cfg, d_cum, d_anc, d_sum, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_filter_move_device(rr_ctx* c, const float* d_states_in, int n, const uint32_t* d_ancestors, int n_out, float Dc, float Ds, float dx, float dy,
                          const rr_filter_config* cfg, float* d_states_out, void* stream)
{
    int rc = check_filter_move(c, "rr_filter_move_device", d_states_in, n, d_ancestors, n_out, Dc, Ds, dx, dy, cfg, d_states_out, 16); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_filter_move(d_states_in, n, d_ancestors, n_out, Dc, Ds, dx, dy, *cfg, d_states_out, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_filter_move(rr_ctx* c, const float* states_in, int n, const uint32_t* ancestors, int n_out, float Dc, float Ds, float dx, float dy,
                   const rr_filter_config* cfg, float* states_out)
{
    int rc = check_filter_move(c, "rr_filter_move", states_in, n, ancestors, n_out, Dc, Ds, dx, dy, cfg, states_out, 4); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    RR_STAGE(c, st);
    float* d_in; uint32_t* d_anc; float* d_out;
    RR_HIP(c, st.up(states_in, (size_t)n * 4, d_in));
    RR_HIP(c, st.up(ancestors, (size_t)n_out, d_anc));
    RR_HIP(c, st.hold(states_out, (size_t)n_out * 4, d_out));
    rc = rr_filter_move_device(c, d_in, n, d_anc, n_out, Dc, Ds, dx, dy, cfg, d_out, c->stream); if (rc) return rc;
    return st.commit();
}

// ---- map refinement (rr_refine.hip) ---------------------------------------------------------------------------------------
void rr_refine_tile_sizes(int* points_tile, int* hyps_per_group, int* row_tile) { refine_tile_sizes(points_tile, hyps_per_group, row_tile); }

int rr_nearest_field_device(rr_ctx* c, const uint8_t* d_occ_u8, int threshold, const rr_field_config* cfg, uint32_t* d_nearest_u32, void* stream)
{
    int rc = check_nearest_field(c, "rr_nearest_field_device", d_occ_u8, threshold, cfg, d_nearest_u32); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_nearest_field(d_occ_u8, threshold, *cfg, d_nearest_u32, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_nearest_field(rr_ctx* c, const uint8_t* occ_u8, int threshold, const rr_field_config* cfg, uint32_t* nearest_u32)
{
    int rc = check_nearest_field(c, "rr_nearest_field", occ_u8, threshold, cfg, nearest_u32); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    uint8_t* d_occ; uint32_t* d_near;
    RR_HIP(c, st.up(occ_u8, cells, d_occ));
    RR_HIP(c, st.hold(nearest_u32, cells, d_near));
    rc = rr_nearest_field_device(c, d_occ, threshold, cfg, d_near, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_refine_poses_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_count, int max_points, const double* d_init, int n_hyp,
                           const uint32_t* d_nearest_u32, const rr_field_config* cfg, int iterations, rr_icp_rec* d_recs, void* stream)
{
    int rc = check_refine_poses(c, "rr_refine_poses_device", d_points, d_count != nullptr, max_points, d_init, n_hyp, d_nearest_u32, cfg, iterations,
                                d_recs); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_refine(d_points, d_count, max_points, d_init, n_hyp, d_nearest_u32, *cfg, iterations, d_recs, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_refine_poses(rr_ctx* c, const rr_radar_point* points, uint32_t count, int max_points, const double* init, int n_hyp,
                    const uint32_t* nearest_u32, const rr_field_config* cfg, int iterations, rr_icp_rec* recs)
{
    int rc = check_refine_poses(c, "rr_refine_poses", points, true, max_points, init, n_hyp, nearest_u32, cfg, iterations, recs); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_hyp, cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    rr_radar_point* d_points; uint32_t* d_count; double* d_init; uint32_t* d_near; rr_icp_rec* d_recs;
    RR_HIP(c, st.up_rows(points, 1, (size_t)max_points, &count, d_points));
    RR_HIP(c, st.up(&count, 1, d_count));
    RR_HIP(c, st.up(init, n * 4, d_init));
    RR_HIP(c, st.up(nearest_u32, cells, d_near));
    RR_HIP(c, st.hold(recs, n, d_recs));
    RR_HIP(c, hipStreamSynchronize(c->stream));        // (count is this call's own variable)
    rc = rr_refine_poses_device(c, d_points, d_count, max_points, d_init, n_hyp, d_near, cfg, iterations, d_recs, c->stream); if (rc) return rc;
    return st.commit();
}

// ---- beam model (rr_cast.hip) -------------------------------------------------------------------------------------------------
void rr_cast_tile_sizes(int* angles_tile, int* hyps_per_wave, int* hyps_per_group) { cast_tile_sizes(angles_tile, hyps_per_wave, hyps_per_group); }

int rr_scan_profile_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points, uint16_t* d_first_bin,
                           void* stream)
{
    int rc = check_scan_profile(c, "rr_scan_profile_device", d_points, d_offsets, n_frames, max_points, d_first_bin); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_scan_profile(d_points, d_offsets, n_frames, max_points, polar_grid(c->cfg), d_first_bin, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_scan_profile(rr_ctx* c, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, uint16_t* first_bin)
{
    int rc = check_scan_profile(c, "rr_scan_profile", points, offsets, n_frames, max_points, first_bin); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_frames;
    RR_STAGE(c, st);
    std::vector<uint32_t> totals; rr_radar_point* d_points; uint32_t* d_offs; uint16_t* d_first;
    rc = up_points(c, st, points, offsets, n, (size_t)max_points, totals, d_points, d_offs); if (rc) return rc;
    RR_HIP(c, st.hold(first_bin, n * (size_t)c->cfg.n_angles, d_first));
    rc = rr_scan_profile_device(c, d_points, d_offs, n_frames, max_points, d_first, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_cast_map_device(rr_ctx* c, const float* d_states, int n_hyp, const float* d_dirs, const uint16_t* d_field_u16, const rr_field_config* cfg,
                       const rr_beam_config* beam, uint16_t* d_ranges, void* stream)
{
    int rc = check_cast(c, "rr_cast_map_device", true, nullptr, d_states, n_hyp, 65535, "1..65535", d_dirs, d_field_u16, cfg, beam, d_ranges != nullptr,
                        d_ranges, nullptr); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_cast(nullptr, d_states, n_hyp, d_dirs, c->cfg.n_angles, c->cfg.resolution, d_field_u16, *cfg, *beam, d_ranges, nullptr, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_cast_map(rr_ctx* c, const float* states, int n_hyp, const float* dirs, const uint16_t* field_u16, const rr_field_config* cfg,
                const rr_beam_config* beam, uint16_t* ranges)
{
    int rc = check_cast(c, "rr_cast_map", true, nullptr, states, n_hyp, 65535, "1..65535", dirs, field_u16, cfg, beam, ranges != nullptr, ranges, nullptr);
    if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_hyp, A = (size_t)c->cfg.n_angles, cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    float* d_states; float* d_dirs; uint16_t* d_field; uint16_t* d_ranges;
    RR_HIP(c, st.up(states, n * 4, d_states));
    RR_HIP(c, st.up(dirs, A * 2, d_dirs));
    RR_HIP(c, st.up(field_u16, cells, d_field));
    RR_HIP(c, st.hold(ranges, n * A, d_ranges));
    rc = rr_cast_map_device(c, d_states, n_hyp, d_dirs, d_field, cfg, beam, d_ranges, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_score_beams_device(rr_ctx* c, const uint16_t* d_first_bin, const float* d_states, int n_hyp, const float* d_dirs, const uint16_t* d_field_u16,
                          const rr_field_config* cfg, const rr_beam_config* beam, rr_beam_rec* d_recs, void* stream)
{
    int rc = check_cast(c, "rr_score_beams_device", d_first_bin != nullptr, d_first_bin, d_states, n_hyp, 1 << 22, "1..2^22", d_dirs, d_field_u16, cfg, beam,
                        d_recs != nullptr, nullptr, d_recs); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_cast(d_first_bin, d_states, n_hyp, d_dirs, c->cfg.n_angles, c->cfg.resolution, d_field_u16, *cfg, *beam, nullptr, d_recs, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_score_beams(rr_ctx* c, const uint16_t* first_bin, const float* states, int n_hyp, const float* dirs, const uint16_t* field_u16,
                   const rr_field_config* cfg, const rr_beam_config* beam, rr_beam_rec* recs)
{
    int rc = check_cast(c, "rr_score_beams", first_bin != nullptr, first_bin, states, n_hyp, 1 << 22, "1..2^22", dirs, field_u16, cfg, beam, recs != nullptr,
                        nullptr, recs); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_hyp, A = (size_t)c->cfg.n_angles, cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    uint16_t* d_first; float* d_states; float* d_dirs; uint16_t* d_field; rr_beam_rec* d_recs;
    RR_HIP(c, st.up(first_bin, A, d_first));
    RR_HIP(c, st.up(states, n * 4, d_states));
    RR_HIP(c, st.up(dirs, A * 2, d_dirs));
    RR_HIP(c, st.up(field_u16, cells, d_field));
    RR_HIP(c, st.hold(recs, n, d_recs));
    rc = rr_score_beams_device(c, d_first, d_states, n_hyp, d_dirs, d_field, cfg, beam, d_recs, c->stream); if (rc) return rc;
    return st.commit();
}

// ---- mesh maps (rr_slice.hip) ---------------------------------------------------------------------------------------------------
void rr_slice_tile_sizes(int* small_cells, int* tile_side, int* group_size) { slice_tile_sizes(small_cells, tile_side, group_size); }

int rr_slice_mesh_device(rr_ctx* c, const rr_slice_config* slice, const rr_field_config* cfg, const uint8_t* d_skip_u8, uint8_t* d_occ_u8,
                         uint32_t* d_object_u32, void* stream)
{
    int rc = check_slice(c, "rr_slice_mesh_device", slice, cfg, d_occ_u8, d_object_u32); if (rc) return rc;
    if (c->n_tris == 0) return 0;                                     // an empty mesh writes nothing
    RR_HIP(c, hipSetDevice(c->device));
    hipStream_t s = stream_of(c, stream);
    Scratch sc(c->scratch_of(s), s);
    uint32_t* list;      // the large list: its counter, then one word per triangle record
    RR_HIP(c, sc.room(slice_scratch_words((size_t)c->n_tris), list));
    launch_slice(reinterpret_cast<const TriRec*>(c->d_bvh.p + c->tri_base4), (size_t)c->n_tris, c->d_rest_v.p, c->d_rest_f.p, c->d_poses.p, d_skip_u8,
                 *slice, *cfg, d_occ_u8, d_object_u32, list, s);
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_slice_mesh(rr_ctx* c, const rr_slice_config* slice, const rr_field_config* cfg, const uint8_t* skip_u8, uint8_t* occ_u8, uint32_t* object_u32)
{
    int rc = check_slice(c, "rr_slice_mesh", slice, cfg, occ_u8, object_u32); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    uint8_t* d_skip; uint8_t* d_occ; uint32_t* d_obj;
    RR_HIP(c, st.up(skip_u8, (size_t)c->n_objects, d_skip));
    RR_HIP(c, st.up(occ_u8, cells, d_occ));                          // the call accumulates
    RR_HIP(c, st.up(object_u32, cells, d_obj));
    rc = rr_slice_mesh_device(c, slice, cfg, d_skip, d_occ, d_obj, c->stream); if (rc) return rc;
    st.out(occ_u8, d_occ, cells);
    st.out(object_u32, d_obj, cells);
    return st.commit();
}

// ---- connected components (rr_components.hip) -------------------------------------------------------------------------------------
void rr_components_tile_sizes(int* tile_w, int* tile_h) { components_tile_sizes(tile_w, tile_h); }

size_t rr_components_scratch_bytes(int n_planes, const rr_components_config* cfg)
{
    if (bad_components_shape(n_planes, cfg)) return 0;
    return components_scratch_bytes((size_t)n_planes, (size_t)cfg->height * cfg->width);
}

int rr_label_components_device(rr_ctx* c, const uint8_t* d_planes_u8, int n_planes, const rr_components_config* cfg, uint32_t* d_labels,
                               uint8_t* d_clean_u8, rr_component* d_comps, uint32_t* d_counts, void* d_scratch, size_t scratch_bytes, void* stream)
{
    const std::string w("rr_label_components_device");
    int rc = check_components(c, w.c_str(), d_planes_u8, n_planes, cfg, d_clean_u8, d_comps, d_counts); if (rc) return rc;
    if (!d_scratch) return fail(c, -3, w + ": null scratch");
    if ((uintptr_t)d_scratch % 16 != 0 || (uintptr_t)d_comps % 16 != 0) return fail(c, -3, w + ": the scratch and the records must be 16-byte aligned");
    if ((uintptr_t)d_labels % 4 != 0 || (uintptr_t)d_counts % 4 != 0) return fail(c, -3, w + ": the label plane and the counts must be 4-byte aligned");
    const size_t need = rr_components_scratch_bytes(n_planes, cfg);
    if (scratch_bytes < need) return fail(c, -3, w + ": scratch of " + std::to_string(scratch_bytes) + " bytes, the call needs " + std::to_string(need));
    RR_HIP(c, hipSetDevice(c->device));
    launch_components(d_planes_u8, n_planes, *cfg, d_labels, d_clean_u8, d_comps, d_counts, d_scratch, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_label_components(rr_ctx* c, const uint8_t* planes_u8, int n_planes, const rr_components_config* cfg, uint32_t* labels, uint8_t* clean_u8,
                        rr_component* comps, uint32_t* counts)
{
    int rc = check_components(c, "rr_label_components", planes_u8, n_planes, cfg, clean_u8, comps, counts); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_planes, npx = (size_t)cfg->height * cfg->width, cap = (size_t)cfg->max_components;
    const size_t scratch = rr_components_scratch_bytes(n_planes, cfg);
    RR_STAGE(c, st);
    uint8_t *d_planes, *d_clean, *d_scratch; uint32_t *d_labels, *d_counts; rr_component* d_comps;
    RR_HIP(c, st.up(planes_u8, n * npx, d_planes));
    RR_HIP(c, st.hold(labels, n * npx, d_labels));
    RR_HIP(c, st.hold(clean_u8, n * npx, d_clean));
    // the records of plane a that exist, min(kept, max_components), and nothing beyond them: the kept totals are every second word of counts
    std::vector<uint32_t> kept(n);
    std::vector<uint32_t> both(2 * n);
    RR_HIP(c, st.hold_rows(comps, n, cap, cap, kept.data(), d_comps));
    RR_HIP(c, st.room(2 * n, d_counts));
    RR_HIP(c, st.room(scratch, d_scratch));
    rc = rr_label_components_device(c, d_planes, n_planes, cfg, d_labels, d_clean, d_comps, d_counts, d_scratch, scratch, c->stream); if (rc) return rc;
    // (the totals come home first, on their own, because the records' scatter reads them)
    RR_HIP(c, hipMemcpyAsync(both.data(), d_counts, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    RR_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t a = 0; a < n; a++) kept[a] = both[2 * a];
    rc = st.commit(); if (rc) return rc;
    std::memcpy(counts, both.data(), 2 * n * sizeof(uint32_t));
    return 0;
}

// ---- correlative scan matching (rr_correlate.hip) ----------------------------------------------------------------------------------
void rr_correlate_tile_sizes(int* points_tile, int* tops_per_wave, int* parents_per_wave)
{
    correlate_tile_sizes(points_tile, tops_per_wave, parents_per_wave);
}

size_t rr_correlate_scratch_bytes(int n_rot, int max_points, const rr_corr_config* cfg)
{
    if (bad_correlate_shape(n_rot, max_points, cfg)) return 0;
    return correlate_scratch_bytes((size_t)n_rot, (size_t)max_points, cfg->levels, (size_t)cfg->capacity);
}

int rr_field_pyramid_device(rr_ctx* c, const uint16_t* d_field_u16, const rr_field_config* cfg, int levels, uint16_t* d_pyramid_u16, void* stream)
{
    int rc = check_pyramid(c, "rr_field_pyramid_device", d_field_u16, cfg, levels, d_pyramid_u16); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    launch_field_pyramid(d_field_u16, *cfg, levels, d_pyramid_u16, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_field_pyramid(rr_ctx* c, const uint16_t* field_u16, const rr_field_config* cfg, int levels, uint16_t* pyramid_u16)
{
    int rc = check_pyramid(c, "rr_field_pyramid", field_u16, cfg, levels, pyramid_u16); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)cfg->width * cfg->height;
    RR_STAGE(c, st);
    uint16_t *d_field, *d_pyramid;
    RR_HIP(c, st.up(field_u16, cells, d_field));
    RR_HIP(c, st.hold(pyramid_u16, ((size_t)levels + 1) * cells, d_pyramid));
    rc = rr_field_pyramid_device(c, d_field, cfg, levels, d_pyramid, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_correlate_scan_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_count, int max_points, const float* d_rot, int n_rot,
                             const uint16_t* d_pyramid_u16, const rr_field_config* cfg, const rr_corr_config* corr, rr_corr_rec* d_rec,
                             void* d_scratch, size_t scratch_bytes, void* stream)
{
    const std::string w("rr_correlate_scan_device");
    int rc = check_correlate(c, w.c_str(), d_points, d_count != nullptr, max_points, d_rot, n_rot, d_pyramid_u16, cfg, corr, d_rec, true); if (rc) return rc;
    if (!d_scratch) return fail(c, -3, w + ": null scratch");
    if ((uintptr_t)d_scratch % 16 != 0) return fail(c, -3, w + ": the scratch must be 16-byte aligned");
    const size_t need = rr_correlate_scratch_bytes(n_rot, max_points, corr);
    if (scratch_bytes < need) return fail(c, -3, w + ": scratch of " + std::to_string(scratch_bytes) + " bytes, the call needs " + std::to_string(need));
    RR_HIP(c, hipSetDevice(c->device));
    launch_correlate(d_points, d_count, max_points, d_rot, n_rot, d_pyramid_u16, *cfg, *corr, d_rec, d_scratch, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_correlate_scan(rr_ctx* c, const rr_radar_point* points, uint32_t count, int max_points, const float* rot, int n_rot, const uint16_t* pyramid_u16,
                      const rr_field_config* cfg, const rr_corr_config* corr, rr_corr_rec* rec)
{
    int rc = check_correlate(c, "rr_correlate_scan", points, true, max_points, rot, n_rot, pyramid_u16, cfg, corr, rec, false); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t cells = (size_t)cfg->width * cfg->height, scratch = rr_correlate_scratch_bytes(n_rot, max_points, corr);
    RR_STAGE(c, st);
    rr_radar_point* d_points; uint32_t* d_count; float* d_rot; uint16_t* d_pyramid; rr_corr_rec* d_rec; uint8_t* d_scratch;
    RR_HIP(c, st.up_rows(points, 1, (size_t)max_points, &count, d_points));
    RR_HIP(c, st.up(&count, 1, d_count));
    RR_HIP(c, st.up(rot, (size_t)n_rot * 4, d_rot));
    RR_HIP(c, st.up(pyramid_u16, ((size_t)corr->levels + 1) * cells, d_pyramid));
    RR_HIP(c, st.hold(rec, 1, d_rec));
    RR_HIP(c, st.room(scratch, d_scratch));
    RR_HIP(c, hipStreamSynchronize(c->stream));        // (count is this call's own variable)
    rc = rr_correlate_scan_device(c, d_points, d_count, max_points, d_rot, n_rot, d_pyramid, cfg, corr, d_rec, d_scratch, scratch, c->stream);
    if (rc) return rc;
    return st.commit();
}

// ---- oriented surface points and point-to-line scan matching (rr_surfels.hip) ------------------------------------------------------
void rr_surfels_tile_sizes(int* points_tile, int* cells_chunk) { surfels_tile_sizes(points_tile, cells_chunk); }

size_t rr_surfels_scratch_bytes(int n_frames, const rr_surfel_config* cfg)
{
    if (bad_surfels_shape(n_frames, cfg)) return 0;
    return surfels_scratch_bytes((size_t)n_frames, (size_t)cfg->width * cfg->width);
}

int rr_surface_points_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points,
                             const rr_surfel_config* cfg, rr_surfel* d_surfels, int max_surfels, uint32_t* d_counts, void* d_scratch,
                             size_t scratch_bytes, void* stream)
{
    const std::string w("rr_surface_points_device");
    int rc = check_surfels(c, w, d_points, d_offsets, n_frames, max_points, cfg, d_surfels, max_surfels, d_counts); if (rc) return rc;
    if (!d_scratch) return fail(c, -3, w + ": null scratch");
    if ((uintptr_t)d_scratch % 16 != 0 || (uintptr_t)d_surfels % 16 != 0) return fail(c, -3, w + ": the scratch and the records must be 16-byte aligned");
    if ((uintptr_t)d_counts % 4 != 0) return fail(c, -3, w + ": the counts must be 4-byte aligned");
    const size_t need = rr_surfels_scratch_bytes(n_frames, cfg);
    if (scratch_bytes < need) return fail(c, -3, w + ": scratch of " + std::to_string(scratch_bytes) + " bytes, the call needs " + std::to_string(need));
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, launch_surface_points(d_points, d_offsets, n_frames, c->cfg.n_angles, max_points, *cfg, d_surfels, max_surfels, d_counts, d_scratch,
                                    stream_of(c, stream)));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_surface_points(rr_ctx* c, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const rr_surfel_config* cfg,
                      rr_surfel* surfels, int max_surfels, uint32_t* counts)
{
    int rc = check_surfels(c, "rr_surface_points", points, offsets, n_frames, max_points, cfg, surfels, max_surfels, counts); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_frames, cap = (size_t)max_surfels, scratch = rr_surfels_scratch_bytes(n_frames, cfg);
    RR_STAGE(c, st);
    std::vector<uint32_t> totals, kept(n), both(2 * n); rr_radar_point* d_points; uint32_t *d_offs, *d_counts; rr_surfel* d_surfels; uint8_t* d_scratch;
    rc = up_points(c, st, points, offsets, n, (size_t)max_points, totals, d_points, d_offs); if (rc) return rc;
    // the records of frame f that exist, min(kept, max_surfels), and nothing beyond them: the kept totals are every second word of counts
    RR_HIP(c, st.hold_rows(surfels, n, cap, cap, kept.data(), d_surfels));
    RR_HIP(c, st.room(2 * n, d_counts));
    RR_HIP(c, st.room(scratch, d_scratch));
    rc = rr_surface_points_device(c, d_points, d_offs, n_frames, max_points, cfg, d_surfels, max_surfels, d_counts, d_scratch, scratch, c->stream);
    if (rc) return rc;
    // (the totals come home first, on their own, because the records' scatter reads them)
    RR_HIP(c, hipMemcpyAsync(both.data(), d_counts, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    RR_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t f = 0; f < n; f++) kept[f] = both[2 * f];
    rc = st.commit(); if (rc) return rc;
    std::memcpy(counts, both.data(), 2 * n * sizeof(uint32_t));
    return 0;
}

// ---- pose-graph optimisation (rr_graph.hip) ---------------------------------------------------------------------------------------
void rr_graph_tile_sizes(int* node_chunk, int* edge_tile) { graph_tile_sizes(node_chunk, edge_tile); }

size_t rr_graph_plan_bytes(int n_nodes, int n_edges)
{
    if (bad_graph_shape(n_nodes, n_edges)) return 0;
    return graph_plan_bytes((size_t)n_nodes, (size_t)n_edges);
}

size_t rr_graph_scratch_bytes(int n_nodes, int n_edges, const rr_graph_config* cfg)
{
    if (bad_graph_shape(n_nodes, n_edges) || bad_graph_config(cfg)) return 0;
    return graph_scratch_bytes((size_t)n_nodes, (size_t)n_edges, (size_t)cfg->cg_iterations);
}

int rr_graph_plan_device(rr_ctx* c, const rr_graph_edge* d_edges, int n_nodes, int n_edges, void* d_plan, size_t plan_bytes, void* stream)
{
    const std::string w("rr_graph_plan_device");
    int rc = check_graph_plan(c, w, d_edges, n_nodes, n_edges, d_plan, plan_bytes); if (rc) return rc;
    if ((uintptr_t)d_edges % 16 != 0 || (uintptr_t)d_plan % 16 != 0) return fail(c, -3, w + ": the edges and the plan must be 16-byte aligned");
    RR_HIP(c, hipSetDevice(c->device));
    RR_HIP(c, launch_graph_plan(d_edges, n_nodes, n_edges, d_plan, stream_of(c, stream)));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_graph_plan(rr_ctx* c, const rr_graph_edge* edges, int n_nodes, int n_edges, void* plan, size_t plan_bytes)
{
    int rc = check_graph_plan(c, "rr_graph_plan", edges, n_nodes, n_edges, plan, plan_bytes); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t need = graph_plan_bytes((size_t)n_nodes, (size_t)n_edges);
    RR_STAGE(c, st);
    rr_graph_edge* d_edges; uint8_t* d_plan;
    RR_HIP(c, st.up(n_edges > 0 ? edges : nullptr, (size_t)n_edges, d_edges));
    RR_HIP(c, st.hold(static_cast<uint8_t*>(plan), need, d_plan));
    rc = rr_graph_plan_device(c, d_edges, n_nodes, n_edges, d_plan, need, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_optimize_graph_device(rr_ctx* c, double* d_states, const uint8_t* d_fixed, const rr_graph_edge* d_edges, int n_nodes, int n_edges,
                             const void* d_plan, const rr_graph_config* cfg, rr_graph_rec* d_recs, uint8_t* d_edge_flags, void* d_scratch,
                             size_t scratch_bytes, void* stream)
{
    const std::string w("rr_optimize_graph_device");
    int rc = check_graph(c, w, d_states, d_fixed, d_edges, n_nodes, n_edges, d_plan, cfg, d_recs); if (rc) return rc;
    if (!d_scratch) return fail(c, -3, w + ": null scratch");
    if ((uintptr_t)d_states % 16 != 0 || (uintptr_t)d_edges % 16 != 0 || (uintptr_t)d_recs % 16 != 0 || (uintptr_t)d_plan % 16 != 0 ||
        (uintptr_t)d_scratch % 16 != 0)
        return fail(c, -3, w + ": the states, the edges, the records, the plan and the scratch must be 16-byte aligned");
    const size_t need = rr_graph_scratch_bytes(n_nodes, n_edges, cfg);
    if (scratch_bytes < need) return fail(c, -3, w + ": scratch of " + std::to_string(scratch_bytes) + " bytes, the call needs " + std::to_string(need));
    RR_HIP(c, hipSetDevice(c->device));
    launch_optimize_graph(d_states, d_fixed, d_edges, n_nodes, n_edges, d_plan, *cfg, d_recs, d_edge_flags, d_scratch, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_optimize_graph(rr_ctx* c, double* states, const uint8_t* fixed, const rr_graph_edge* edges, int n_nodes, int n_edges, const void* plan,
                      const rr_graph_config* cfg, rr_graph_rec* recs, uint8_t* edge_flags)
{
    int rc = check_graph(c, "rr_optimize_graph", states, fixed, edges, n_nodes, n_edges, plan, cfg, recs); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t N = (size_t)n_nodes, E = (size_t)n_edges, scratch = rr_graph_scratch_bytes(n_nodes, n_edges, cfg);
    RR_STAGE(c, st);
    double* d_states; uint8_t *d_fixed, *d_plan, *d_flags, *d_scratch; rr_graph_edge* d_edges; rr_graph_rec* d_recs;
    RR_HIP(c, st.up(static_cast<const double*>(states), 4 * N, d_states));
    st.out(states, static_cast<const double*>(d_states), 4 * N);
    RR_HIP(c, st.up(fixed, N, d_fixed));
    RR_HIP(c, st.up(n_edges > 0 ? edges : nullptr, E, d_edges));
    RR_HIP(c, st.up(static_cast<const uint8_t*>(plan), graph_plan_bytes(N, E), d_plan));
    RR_HIP(c, st.hold(recs, (size_t)cfg->iterations + 1, d_recs));
    RR_HIP(c, st.hold(n_edges > 0 ? edge_flags : nullptr, E, d_flags));
    RR_HIP(c, st.room(scratch, d_scratch));
    rc = rr_optimize_graph_device(c, d_states, d_fixed, d_edges, n_nodes, n_edges, d_plan, cfg, d_recs, d_flags, d_scratch, scratch, c->stream);
    if (rc) return rc;
    return st.commit();
}

// ---- object annotations (rr_notes.hip) --------------------------------------------------------------------------------
size_t rr_annotate_scratch_bytes(int n_frames, int n_objects, int n_angles)
{
    if (n_frames < 1 || n_objects < 1 || n_angles < 1) return 0;
    return note_scratch_bytes((size_t)n_frames, (size_t)n_objects, n_angles);
}

int rr_annotate_labels_device(rr_ctx* c, const uint32_t* d_labels, const uint8_t* d_imgs_u8, int n_frames, int n_objects, uint32_t extent_mask,
                              rr_object_note* d_notes, uint32_t* d_skipped, void* d_scratch, size_t scratch_bytes, void* stream)
{
    const std::string w("rr_annotate_labels_device");
    int rc = check_annotate(c, w.c_str(), d_labels, n_frames, 65535, n_objects, extent_mask, d_notes, d_skipped); if (rc) return rc;
    if (!d_scratch) return fail(c, -3, w + ": null scratch");
    if ((uintptr_t)d_scratch % 16 != 0 || (uintptr_t)d_notes % 16 != 0) return fail(c, -3, w + ": the scratch and the records must be 16-byte aligned");
    const rr_config& g = c->cfg;
    const size_t need = note_scratch_bytes((size_t)n_frames, (size_t)n_objects, g.n_angles);
    if (scratch_bytes < need) return fail(c, -3, w + ": scratch of " + std::to_string(scratch_bytes) + " bytes, the call needs " + std::to_string(need));
    RR_HIP(c, hipSetDevice(c->device));
    launch_notes(d_labels, d_imgs_u8, n_frames, (uint32_t)n_objects, extent_mask, polar_grid(g), d_notes, d_skipped, d_scratch, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_annotate_labels(rr_ctx* c, const uint32_t* labels, const uint8_t* imgs_u8, int n_frames, int n_objects, uint32_t extent_mask,
                       rr_object_note* out_notes, uint32_t* out_skipped)
{
    int rc = check_annotate(c, "rr_annotate_labels", labels, n_frames, 65535, n_objects, extent_mask, out_notes, out_skipped); if (rc) return rc;
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n = (size_t)n_frames, n_rec = n * (size_t)n_objects;
    const size_t scratch = note_scratch_bytes(n, (size_t)n_objects, c->cfg.n_angles);
    RR_STAGE(c, st);
    uint32_t *d_labels, *d_skipped; uint8_t *d_imgs, *d_scratch; rr_object_note* d_notes;
    RR_HIP(c, st.up(labels, n * npx, d_labels));
    RR_HIP(c, st.up(imgs_u8, n * npx, d_imgs));
    RR_HIP(c, st.hold(out_notes, n_rec, d_notes));
    RR_HIP(c, st.hold(out_skipped, n, d_skipped));
    RR_HIP(c, st.room(scratch, d_scratch));
    rc = rr_annotate_labels_device(c, d_labels, d_imgs, n_frames, n_objects, extent_mask, d_notes, d_skipped, d_scratch, scratch, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_label_points_device(rr_ctx* c, const rr_radar_point* d_points, const uint32_t* d_offsets, int n_frames, int max_points, const uint32_t* d_labels,
                           const uint32_t* d_faces, const float* d_vel_img, uint32_t* d_point_labels, uint32_t* d_point_faces, float* d_point_vel,
                           void* stream)
{
    const std::string w("rr_label_points_device");
    int rc = check_planes(c, w, d_points && d_offsets && d_labels && d_point_labels, n_frames, 65535); if (rc) return rc;
    if (max_points < 0) return fail(c, -3, w + ": max_points must be >= 0");
    if (!d_faces != !d_point_faces) return fail(c, -3, w + ": the face plane and the points' faces come together or not at all");
    if (!d_vel_img != !d_point_vel) return fail(c, -3, w + ": the velocity image and the points' range rates come together or not at all");
    if (max_points == 0) return 0;
    RR_HIP(c, hipSetDevice(c->device));
    launch_label_points(d_points, d_offsets, n_frames, max_points, d_labels, d_faces, d_vel_img, d_point_labels, d_point_faces, d_point_vel,
                        c->cfg.n_cells, c->cfg.n_angles, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_polar_to_cartesian_labels_device(rr_ctx* c, const uint32_t* d_planes_u32, int n_frames, const rr_cartesian_config* cfg, uint32_t* d_cart_u32,
                                        void* stream)
{
    int rc = check_cartesian(c, "rr_polar_to_cartesian_labels_device", d_planes_u32, n_frames, cfg, d_cart_u32); if (rc) return rc;
    if (cfg->interpolation != 0) return fail(c, -3, "rr_polar_to_cartesian_labels_device: interpolation must be 0 (nearest): ids do not interpolate");
    RR_HIP(c, hipSetDevice(c->device));
    launch_cartesian_labels(d_planes_u32, n_frames, *cfg, polar_grid(c->cfg), d_cart_u32, stream_of(c, stream));
    RR_HIP(c, hipGetLastError());
    return 0;
}

int rr_polar_to_cartesian_labels(rr_ctx* c, const uint32_t* planes_u32, int n_frames, const rr_cartesian_config* cfg, uint32_t* cart_u32)
{
    int rc = check_cartesian(c, "rr_polar_to_cartesian_labels", planes_u32, n_frames, cfg, cart_u32); if (rc) return rc;
    if (cfg->interpolation != 0) return fail(c, -3, "rr_polar_to_cartesian_labels: interpolation must be 0 (nearest): ids do not interpolate");
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n = (size_t)n_frames, n_out = n * cfg->width * cfg->width;
    RR_STAGE(c, st);
    uint32_t *d_planes, *d_cart;
    RR_HIP(c, st.up(planes_u32, n * npx, d_planes));
    RR_HIP(c, st.hold(cart_u32, n_out, d_cart));
    rc = rr_polar_to_cartesian_labels_device(c, d_planes, n_frames, cfg, d_cart, c->stream); if (rc) return rc;
    return st.commit();
}

int rr_simulate_batch_annotations(rr_ctx* c, const float* poses, int n_frames, uint32_t extent_mask, uint8_t* out_imgs_u8, rr_object_note* out_notes,
                                  uint32_t* out_skipped)
{
    // refused before anything is simulated (the context stands in for the planes: they are its own)
    int rc = check_annotate(c, "rr_simulate_batch_annotations", c, n_frames, RR_MAX_BATCH, c ? (long long)c->n_objects : 1, extent_mask, out_notes, out_skipped);
    if (rc) return rc;
    rc = check_ready(c); if (rc) return rc;
    if (!poses) return fail(c, -3, "rr_simulate_batch_annotations: null poses");
    RR_HIP(c, hipSetDevice(c->device));
    const size_t npx = (size_t)c->cfg.n_cells * c->cfg.n_angles, n = (size_t)n_frames, n_obj = c->n_objects, n_rec = n * n_obj;
    const size_t scratch = note_scratch_bytes(n, n_obj, c->cfg.n_angles);
    RR_STAGE(c, st);
    uint32_t *d_labels, *d_skipped; uint8_t *d_imgs, *d_scratch; rr_object_note* d_notes;
    RR_HIP(c, st.room(n * npx, d_imgs));
    RR_HIP(c, st.room(n * npx, d_labels));
    RR_HIP(c, st.hold(out_notes, n_rec, d_notes));
    RR_HIP(c, st.hold(out_skipped, n, d_skipped));
    RR_HIP(c, st.room(scratch, d_scratch));
    rc = rr_simulate_batch_provenance_device(c, poses, n_frames, d_imgs, d_labels, nullptr, nullptr, 0, nullptr, c->stream); if (rc) return rc;
    rc = rr_annotate_labels_device(c, d_labels, d_imgs, n_frames, (int)n_obj, extent_mask, d_notes, d_skipped, d_scratch, scratch, c->stream); if (rc) return rc;
    st.out(out_imgs_u8, d_imgs, n * npx, false);
    return st.commit(frame_gate(c));
}

}  // extern "C"
