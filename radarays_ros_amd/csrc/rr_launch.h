// rr_launch.h -- every launcher of rr_kernels.hip, rr_labels.hip, rr_paths.hip, rr_doppler.hip, rr_refit.hip, rr_detect.hip, rr_window.hip, rr_deskew.hip, rr_icp.hip, rr_field.hip, rr_occupancy.hip, rr_filter.hip, rr_refine.hip, rr_cast.hip, rr_slice.hip, rr_components.hip, rr_notes.hip, rr_metrics.hip, rr_align.hip, rr_shift.hip, rr_place.hip and rr_lbvh.hip, declared ONCE: included where they
// are defined (a definition that drifts from its declaration fails there) and where they are called.  Default arguments live here only.
#pragma once
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_polar.h"
#include <hip/hip_ext.h>
#include <string>

namespace rr {
// One launch, with or without the timing events.  ev_start / ev_stop (timing mode) take the dispatch's own begin / end
// timestamps -- what rocprofv3 reports as the kernel's duration -- not the time the launch spent waiting for CUs held by the
// kernels of other streams
template <typename... KArgs, typename... Args>
inline void launch_k(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop,
                     const Args&... args)
{
    if (!ev_start) hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    else hipExtLaunchKernelGGL(kernel, grid, block, lds, s, ev_start, ev_stop, 0, args...);
}

void launch_trace(const Params& P, int pass, const PoseArgs* poses, bool stats, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr,
                  hipEvent_t ev_rep_start = nullptr, hipEvent_t ev_rep_stop = nullptr, bool* repair_launched = nullptr);
void launch_shade(const Params& P, int pass, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void launch_scan(const Params& P, int pass, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void launch_column(const Params& P, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void launch_decay_table(float* decay, int n_cells, double resolution, double energy_loss, hipStream_t s);
void launch_assemble_u8(const uint8_t* cols, uint8_t* img, int n_angles, int n_cells, int scroll, hipStream_t s,
                        int n_loc = 0, size_t block_stride = 0, int n_frames = 1, size_t frame_stride = 0);
void launch_assemble_f32(const float* cols, float* img, int n_angles, int n_cells, int scroll, hipStream_t s);
void launch_assemble_u32(const uint32_t* cols, uint32_t* img, int n_angles, int n_cells, int scroll, hipStream_t s, int n_frames = 1);
// rr_labels.hip (echo provenance).  launch_label: n_seg lists of `stride` records each -> two columns [n_seg][n_cells]; w null: no denoiser
void launch_echo_gather(const Params& P, int pass, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void launch_label(const EchoSrc* lists, const uint32_t* counts, size_t stride, int n_seg, int n_cells, int W, int mode, const float* w,
                  uint32_t* label_cols, uint32_t* face_cols, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void launch_echo_export(const EchoSrc* lists, const uint32_t* counts, size_t cap, int n_seg, rr_echo_src* dst, size_t stride, uint32_t* dst_counts,
                        hipStream_t s);
// rr_paths.hip (wave paths): one record per ray-cast wave of the pass into the caller's rows
void launch_wave_gather(const Params& P, int pass, const WaveOut& W, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// rr_doppler.hip (Doppler): per pass the range rate of every echo; behind the chain the shifted list and the winner's rate per bin
void launch_rate_gather(const Params& P, int pass, const DopArgs& D, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void launch_doppler_shift(const Params& P, const DopArgs& D, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
void launch_vel_winner(const Params& P, const DopArgs& D, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
bool build_bvh4_gpu(const float* verts, size_t nv, const uint32_t* faces, size_t nf, const uint32_t* face_object,
                    Node4** d_nodes_out, size_t* n_nodes_out, TriRec** d_tris_out, size_t* n_tris_out,
                    uint32_t* depth_out, uint32_t* stack_need_out, float* inflate_out,
                    std::string& err, hipStream_t stream);
void launch_debug_trace(const Params& P, const float* origs, const float* dirs, int n,
                        float* out_t, uint32_t* out_face, hipStream_t s, unsigned long long* steps = nullptr);
void launch_encode_refs(Node4* nodes, size_t n_nodes, uint32_t tri_base4, hipStream_t s, size_t n_tris);
// rr_refit.hip (dynamic scenes)
int refit_reduce_groups();
void launch_refit_extent(const TriRec* tris, size_t n, const float* verts, const uint32_t* faces, const float* poses,
                         float* out8, hipStream_t s);
void launch_refit_tris(TriRec* tris, size_t n, const float* verts, const uint32_t* faces, const float* poses, hipStream_t s);
void launch_refit_levels(float4* base4, const uint32_t* level_nodes, const uint32_t* level_off, int n_levels, float inflate,
                         const float4* built4, const uint8_t* moved, float extra, hipStream_t s);
void launch_tree_cost(const Node4* nodes, size_t n_nodes, double* out, hipStream_t s);
void launch_gather_refs(const Node4* nodes, size_t n_nodes, uint32_t* out, hipStream_t s);
void launch_pose_soup(const TriRec* tris, size_t n, const float* verts, const uint32_t* faces, const float* poses,
                      float* soup, uint32_t* obj, hipStream_t s);
void launch_mat_limits(const float4* materials, size_t n, double* limits, hipStream_t s);
void* trace0_kernel(bool spill, bool stackless);
void launch_score(const uint8_t* imgs, const uint8_t* ref, size_t npx, int n_images, unsigned long long* sse, hipStream_t s);
// rr_detect.hip (point clouds and Cartesian images)
void launch_detect(const uint8_t* imgs, int n_frames, const rr_detect_config& cfg, const PolarGrid& G, rr_radar_point* points, int max_points,
                   uint32_t* offsets, hipStream_t s);
void launch_cartesian(const uint8_t* imgs, int n_frames, const rr_cartesian_config& cfg, const PolarGrid& G, uint8_t* out, hipStream_t s);
void launch_detect_scan(uint32_t* offsets /*[n_frames][n_angles + 1]*/, int n_frames, int n_angles, hipStream_t s);
// rr_window.hip (windowed CFAR).  No scratch and no context memory: a count pass into offsets, launch_detect_scan, an emit pass; mask
// [n_frames][n_cells][n_angles] or null is written whole by the count pass.  tile: (rows, columns, halo rows, halo columns), whatever the base's alignment
bool window_tile_sizes(const rr_window_detect_config& cfg, int n_cells, int n_angles, int out[4]);
hipError_t launch_detect_window(const uint8_t* imgs, int n_frames, const rr_window_detect_config& cfg, const PolarGrid& G, rr_radar_point* points,
                                int max_points, uint32_t* offsets, uint8_t* mask, hipStream_t s);
// rr_deskew.hip (sweep compensation).  table [n_frames][n_angles], 16-byte aligned; n_angles * 32 bytes of LDS per workgroup of launch_cartesian_sweep
void launch_sweep_table(const float* az_poses, const float* ref_poses, const float* sensor_vel, float gain, int n_frames, const PolarGrid& G,
                        rr_sweep_rec* table, hipStream_t s);
void launch_compensate_points(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const rr_sweep_rec* table,
                              rr_radar_point* out, const PolarGrid& G, hipStream_t s);
void launch_cartesian_sweep(const uint8_t* imgs, int n_frames, const rr_cartesian_config& cfg, const PolarGrid& G, const rr_sweep_rec* table,
                            int iterations, uint8_t* out, hipStream_t s);
// rr_icp.hip (scan matching: one matcher, point-to-point against a cloud and point-to-line against surface points).  acc: icp_scratch_words /
// line_scratch_words(n_frames) int64 words, zeroed by the first launch; recs and init 8-byte, a surfel target 16-byte aligned
void icp_tile_sizes(int* source_tile, int* target_tile);
size_t icp_scratch_words(size_t n_frames);
void launch_icp(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points, const rr_radar_point* tgt,
                const uint32_t* tgt_count, int max_tgt, const double* init, float gate, int iterations, rr_icp_rec* recs, uint32_t* corr,
                long long* acc, hipStream_t s);
size_t line_scratch_words(size_t n_frames);
void launch_register_surfels(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points, const rr_surfel* tgt,
                             const uint32_t* tgt_count, int max_tgt, const double* init, float gate, int iterations, rr_icp_rec* recs,
                             uint32_t* corr, long long* acc, hipStream_t s);
// rr_field.hip (likelihood field).  No scratch: occ is only ever written with ones, field is written whole, every record of recs is written;
// states of the rasteriser 8-byte aligned or null, recs 8-byte aligned, field must not alias occ
void field_tile_sizes(int* points_tile, int* hyps_per_group, int* row_tile);
void launch_field_raster(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points, const double* states,
                         const rr_field_config& g, uint8_t* occ, hipStream_t s);
void launch_distance_field(const uint8_t* occ, int threshold, const rr_field_config& g, uint16_t* field, hipStream_t s);
void launch_field_score(const rr_radar_point* points, const uint32_t* count, int max_points, const float* states, int n_hyp, const uint16_t* field,
                        const rr_field_config& g, rr_field_rec* recs, hipStream_t s);
// rr_occupancy.hip (occupancy mapping).  No scratch: profile [n_frames][n_angles] is written whole, evidence is accumulated into; states 8-byte
// aligned or null, profile and evidence 4-byte aligned.  Three launches (profile, free space, hits) and one
void occupancy_tile_sizes(int* cells_per_group, int* cells_per_thread, int* scan_chunk);
void launch_occupancy_update(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const double* states,
                             const rr_field_config& g, const rr_occupancy_config& o, const PolarGrid& G, float* profile, int32_t* evidence,
                             hipStream_t s);
void launch_occupancy_map(const int32_t* evidence, const rr_field_config& g, uint8_t* occ, hipStream_t s);
// rr_filter.hip (particle filter step).  No scratch: cum [n] is the scan's only room and an output; recs, cum and summary 8-byte aligned, the states
// 16-byte aligned and apart.  Six launches (start values, minimum, tile sums, their scan by one workgroup, cum, draws) and one
void filter_tile_sizes(int* scan_tile, int* draws_per_group, int* search_tile);
void launch_filter_resample(const rr_field_rec* recs, int n, const uint16_t* table, int n_out, const rr_filter_config& f, uint64_t* cum,
                            uint32_t* ancestors, rr_filter_summary* summary, hipStream_t s);
void launch_filter_move(const float* states_in, int n, const uint32_t* ancestors, int n_out, float Dc, float Ds, float dx, float dy,
                        const rr_filter_config& f, float* states_out, hipStream_t s);
// rr_refine.hip (map refinement).  No scratch and no context memory: nearest [height][width] is written whole (pass A leaves its offsets in it,
// pass B overwrites them), every record of recs is written; init and recs 8-byte aligned, nearest 4-byte aligned and apart from occ.  Two
// launches (columns, rows) and ONE, whatever the iteration count
void refine_tile_sizes(int* points_tile, int* hyps_per_group, int* row_tile);
void launch_nearest_field(const uint8_t* occ, int threshold, const rr_field_config& g, uint32_t* nearest, hipStream_t s);
void launch_refine(const rr_radar_point* points, const uint32_t* count, int max_points, const double* init, int n_hyp, const uint32_t* nearest,
                   const rr_field_config& g, int iterations, rr_icp_rec* recs, hipStream_t s);
// rr_cast.hip (beam model).  No scratch and no context memory: first_bin [n_frames][n_angles] is written whole; launch_cast writes every record
// of recs (the score form: first_bin is ONE profile) or, with recs null, ranges [n_hyp][n_angles] whole.  ONE launch each
void cast_tile_sizes(int* angles_tile, int* hyps_per_wave, int* hyps_per_group);
void launch_scan_profile(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const PolarGrid& G, uint16_t* first_bin,
                         hipStream_t s);
void launch_cast(const uint16_t* first_bin, const float* states, int n_hyp, const float* dirs, int n_angles, double resolution, const uint16_t* field,
                 const rr_field_config& g, const rr_beam_config& bc, uint16_t* ranges, rr_beam_rec* recs, hipStream_t s);
// rr_slice.hip (mesh maps).  occ is only ever written with ones, objects (or null) only ever lowered.  scratch: slice_scratch_words uint32 words for n records
// (the large list's counter, zeroed on s by the call, then the list); skip [n_objects] or null.  A memset and two launches
void slice_tile_sizes(int* small_cells, int* tile_side, int* group_size);
int slice_large_groups();
size_t slice_scratch_words(size_t n_records);
void launch_slice(const TriRec* tris, size_t n, const float* verts, const uint32_t* faces, const float* poses, const uint8_t* skip,
                  const rr_slice_config& sc, const rr_field_config& g, uint8_t* occ, uint32_t* objects, uint32_t* scratch, hipStream_t s);
// rr_components.hip (connected components).  scratch: components_scratch_bytes, 16-byte aligned like comps; its contents before the call do not matter.
// labels (or null: the link plane lives in the scratch), clean (or null), comps (null iff max_components == 0); totals [n_planes][2].  Eight launches
void components_tile_sizes(int* tile_w, int* tile_h);
size_t components_scratch_bytes(size_t n_planes, size_t npx);
void launch_components(const uint8_t* planes, int n_planes, const rr_components_config& cfg, uint32_t* labels, uint8_t* clean, rr_component* comps,
                       uint32_t* totals, void* scratch, hipStream_t s);
// rr_correlate.hip (correlative scan matching).  No context memory.  pyramid [levels + 1][height][width] is written whole (plane 0 only when it is
// not the field itself): levels + 1 launches.  scratch: correlate_scratch_bytes, 16-byte aligned like rec; its contents before the call do not
// matter.  levels + 5 launches, every one below the top level sized by the capacity
void correlate_tile_sizes(int* points_tile, int* tops_per_wave, int* parents_per_wave);
size_t correlate_scratch_bytes(size_t n_rot, size_t max_points, int levels, size_t capacity);
void launch_field_pyramid(const uint16_t* field, const rr_field_config& g, int levels, uint16_t* pyramid, hipStream_t s);
void launch_correlate(const rr_radar_point* points, const uint32_t* count, int max_points, const float* rot, int n_rot, const uint16_t* pyramid,
                      const rr_field_config& g, const rr_corr_config& c, rr_corr_rec* rec, void* scratch, hipStream_t s);
// rr_surfels.hip (oriented surface points).  scratch: surfels_scratch_bytes for n_cells = width * width, 16-byte aligned
// like surfels (null iff max_surfels == 0); its contents before the call do not matter; counts [n_frames][2].  A memset (its error is returned) and
// four launches
void surfels_tile_sizes(int* points_tile, int* cells_chunk);
size_t surfels_scratch_bytes(size_t n_frames, size_t n_cells);
hipError_t launch_surface_points(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int n_angles, int max_points,
                                 const rr_surfel_config& cfg, rr_surfel* surfels, int max_surfels, uint32_t* counts, void* scratch, hipStream_t s);
// rr_graph.hip (pose-graph optimisation).  plan: graph_plan_bytes, scratch: graph_scratch_bytes, states, edges and recs 16-byte aligned; every
// byte of the plan is written (two memsets, whose error is returned, and six launches); the scratch's contents before the call do not matter.
// edges may be null iff n_edges == 0.  Per outer iteration 4 + 2 * cg_iterations launches, then a linearisation and a record
void graph_tile_sizes(int* node_chunk, int* edge_tile);
size_t graph_plan_bytes(size_t n_nodes, size_t n_edges);
size_t graph_scratch_bytes(size_t n_nodes, size_t n_edges, size_t cg_iterations);
hipError_t launch_graph_plan(const rr_graph_edge* edges, int n_nodes, int n_edges, void* plan, hipStream_t s);
void launch_optimize_graph(double* states, const uint8_t* fixed, const rr_graph_edge* edges, int n_nodes, int n_edges, const void* plan,
                           const rr_graph_config& cfg, rr_graph_rec* recs, uint8_t* edge_flags, void* scratch, hipStream_t s);
// rr_notes.hip (object annotations).  scratch: note_scratch_bytes, 16-byte aligned like notes; every word of it, of notes and of skipped is written by the launches
size_t note_scratch_bytes(size_t n_frames, size_t n_objects, int n_angles);
void launch_notes(const uint32_t* labels, const uint8_t* imgs, int n_frames, uint32_t n_objects, uint32_t extent_mask, const PolarGrid& G,
                  rr_object_note* notes, uint32_t* skipped, void* scratch, hipStream_t s);
void launch_label_points(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const uint32_t* labels, const uint32_t* faces,
                         const float* vel, uint32_t* p_labels, uint32_t* p_faces, float* p_vel, int n_cells, int n_angles, hipStream_t s);
void launch_cartesian_labels(const uint32_t* planes, int n_frames, const rr_cartesian_config& cfg, const PolarGrid& G, uint32_t* out, hipStream_t s);
// rr_metrics.hip (images against one reference image).  hist_shape 0: workgroup-private LDS histograms, 1: global atomics
void launch_joint_hist(const uint8_t* imgs, const uint8_t* ref, size_t npx, int n_images, uint32_t* hist, int hist_shape, hipStream_t s);
int ssim_blocks(int n_cells, int n_angles, int win);          // workgroups (= f64 partials) per image of launch_ssim
void launch_ssim(const uint8_t* imgs, const uint8_t* ref, int n_cells, int n_angles, int win, int n_images, double* partial, hipStream_t s);
void launch_metrics_finish(const uint32_t* hist, const double* ssim_part, int n_blocks, double ssim_count, const unsigned long long* sse,
                           size_t npx, rr_image_metrics* out, int n_images, hipStream_t s);
// rr_align.hip (azimuth registration).  sums [n_images + 1][2] and curve [n_images][n_angles] must be zero before their launches
void launch_align_sums(const uint8_t* imgs, const uint8_t* ref, int n_cells, int n_angles, int cell_begin, int cell_end, int n_images,
                       unsigned long long* sums, hipStream_t s);
void launch_align_gram(const uint8_t* imgs, const uint8_t* ref, int n_cells, int n_angles, int cell_begin, int cell_end, int n_images,
                       long long* curve, hipStream_t s);
void launch_align_finish(long long* curve, const unsigned long long* sums, int n_images, int n_angles, int cell_begin, int cell_end,
                         rr_align_record* out, hipStream_t s);
// rr_shift.hip (translation registration).  col [2S+1][W][2] and box [2S+1][2S+1][2] are written whole; sums [n_images][2] and surf
// [n_images][2S+1][2S+1] must be zero before their launches; sse [n_images][2S+1][2S+1] or null
void launch_shift_box(const uint8_t* ref, int H, int W, int S, unsigned long long* col, unsigned long long* box, hipStream_t s);
void launch_shift_sums(const uint8_t* imgs, int H, int W, int S, int n_images, unsigned long long* sums, hipStream_t s);
void launch_shift_gram(const uint8_t* imgs, const uint8_t* ref, int H, int W, int S, int n_images, long long* surf, hipStream_t s);
void launch_shift_finish(long long* surf, unsigned long long* sse, const unsigned long long* sums, const unsigned long long* box, int H, int W,
                         int S, int n_images, rr_shift_record* out, hipStream_t s);
// rr_place.hip (place recognition).  rolls [n_query * S][place_kpad]; keys and aux [n_query][n_candidates] of one database chunk whose first
// candidate has the database index index_base; part [n_query][place_slices(n_candidates)][top_k]; old_* / win* [n_query][top_k] (old_keys ~0
// before the first chunk); d_sse / d_shift [n_query][n_db] or null
void launch_place_describe(const uint8_t* imgs, int n_images, int n_cells, int n_angles, const rr_place_config& p, uint8_t* desc, hipStream_t s);
int place_kpad(int n_rings, int n_sectors);
size_t place_slices(size_t n_candidates);
void launch_place_rolls(const uint8_t* query, int n_query, int n_rings, int n_sectors, uint8_t* rolls, uint32_t* qsums, hipStream_t s);
void launch_place_match(const uint8_t* rolls, const uint32_t* qsums, int n_query, const uint8_t* db, size_t n_candidates, size_t index_base,
                        int n_rings, int n_sectors, unsigned long long* keys, unsigned long long* aux, uint32_t* d_sse, uint16_t* d_shift, size_t n_db,
                        hipStream_t s);
void launch_place_topk(const unsigned long long* keys, const unsigned long long* aux, int n_query, size_t n_candidates, size_t index_base, int top_k,
                       unsigned long long* part, const unsigned long long* old_keys, const unsigned long long* old_aux, unsigned long long* win,
                       unsigned long long* win_aux, hipStream_t s);
void launch_place_finish(const unsigned long long* win, const unsigned long long* win_aux, const uint32_t* qsums, int n_query, int top_k, int n_rings,
                         int n_sectors, rr_place_match* out, hipStream_t s);
void launch_copy_host(const void* src, void* dst, size_t bytes, int blocks, int xcd, hipStream_t s);
void launch_copy_words(const void* src, void* dst, size_t bytes, hipStream_t s);
void launch_debug_brdf(size_t n, const float* in, int model, float* out, hipStream_t s);
void launch_store_u32(const uint32_t* src, uint32_t* h_dst, hipStream_t s);
void launch_debug_fresnel(size_t n, const float* normals, const float* dirs, const double* energy, const double* v1, const float* v2,
                          float* out_rdir, double* out_re, float* out_tdir, double* out_te, hipStream_t s);
}  // namespace rr
