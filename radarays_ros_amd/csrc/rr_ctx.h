// rr_ctx.h -- the context as the library's host files share it (rr_api.hip, rr_scene.hip, rr_frame.hip, rr_side.hip, rr_sets.hip, rr_images.hip, rr_probe.hip): rr_ctx and its
// lanes, the error / timing / roctx helpers, the helpers that cross a file boundary.  Nothing here is public: the interface is include/radarays_mi355.h.
#pragma once
#include "rr_devbuf.h"
#include "rr_launch.h"
#include "rr_sdma.h"
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace rr {
struct KernelTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double total_ms = 0.0;
    uint64_t launches = 0;
    std::vector<float> samples_ms;   // every launch since the last reset (median / percentiles)
};

// a copy to host memory that may still be in flight (wait_delivery): where it goes, the SDMA job that carries it (0: a
// stream-ordered copy, complete once `ev` is) -- and, in a lane's delivery slot, the image buffer it reads
struct Delivery {
    DevBuf<uint8_t> img;
    hipEvent_t ev = nullptr;
    const void* dst = nullptr;     // nullptr: nothing in flight
    uint64_t job = 0;
};

// the room of a host form's round trip and of a device form's scratch (rr_stage.h): anonymous buffers that only grow, slot i for a call's i-th request
using StagePool = std::vector<DevBuf<uint4>>;

struct Lane {
    int buf_seg = 0, buf_cap = 0, buf_sigcap = 0, buf_cells = 0, buf_passes = 0;
    DevBuf<float4> d_wA[2], d_wB[2];
    DevBuf<double2> d_wC[2];
    DevBuf<uint32_t> d_idx[2], d_count[2], d_refpos, d_sig_count, d_spill;
    DevBuf<uint2> d_torder[2], d_sorder;
    DevBuf<uint32_t> d_n_air;
    DevBuf<uint2> d_hit;
    DevBuf<uint8_t> d_cflag, d_cols_u8;
    DevBuf<SigRec> d_sigtmp, d_sig;
    DevBuf<float> d_cols_f32;
    DevBuf<Counters> d_counters;
    DevBuf<uint32_t> d_sticky;    // error bits of ALL frames since the last rr_synchronize (async entry points); the synchronous entry points clear them when they report an error themselves
    DevBuf<float> d_img_f32;
    DevBuf<SegStats> d_seg_stats;
    DevBuf<float4> d_matsets;     // material sets of a parameter batch [n_sets][n_materials]
    DevBuf<double> d_matset_limits;   // ... and their angles of total reflection (k_mat_limits)
    // ... and its beam tables [n_groups][n_beam] with their two trace orders; the host arrays they are copied from stay
    // alive with the lane (a copy from pageable memory may still be staged when the call returns)
    DevBuf<float4> d_set_beams; DevBuf<uint32_t> d_set_order, d_set_order2;
    std::vector<float4> h_set_beams, h_matsets; std::vector<uint32_t> h_set_order, h_set_order2;
    int last_n_seg = 0, last_n_passes = 0;
    int spill_stride = 0, stack_lds = 1;
    // tight later-pass trace grids (rr_device.h: GridHint): the lane's history / overflow counters, the overflow lists,
    // and the page-locked copy of the history that arrives behind every batch (read without a fence: it is a hint)
    DevBuf<GridHint> d_hint; DevBuf<uint32_t> d_ovf_list; int ovf_stride = 0;
    uint32_t* h_hist = nullptr; int hist_gen = 0;
    // Launch graphs (round 5): the launch chain of a batch -- n_reflections x {trace [+ repair], shade, scan}, column, history
    // copy -- captured once per (azimuth block, frames, output buffer, trace rows) and replayed with ONE hipGraphLaunch; the
    // poses are the only thing that changes between replays (the third argument of the pass-0 trace node).  Host time per
    // chain: 46 us launched kernel by kernel (16 launches) against ~11 us replayed (tools/cpp_bench.cpp graph)
    struct FrameGraph {
        int az_begin = 0, az_end = 0, n_frames = 0; const void* cols = nullptr; unsigned short rows[kMaxPasses] = {};
        hipGraph_t g = nullptr; hipGraphExec_t ge = nullptr; hipGraphNode_t pose_node = nullptr; uint64_t last_use = 0; int hits = 0;
        // Replays must not touch a launch that is still queued or running: whether hipGraphExecKernelNodeSetParams rewrites the
        // kernel arguments of an exec IN PLACE is the runtime's business (advisor, round 5: lane reuse is ordered on the device
        // only, the host never waits), so the library does not depend on it -- TWO execs per shape, used alternately, each with
        // an event behind its last launch; the host waits for that event before it re-sets the exec's poses or destroys it.
        // The exec about to be updated was launched two uses of this shape ago: the wait is over before it starts, except for a
        // caller that runs more than a whole lane rotation ahead of the GPU
        hipGraphExec_t ge2 = nullptr; hipEvent_t ev[2] = { nullptr, nullptr }; bool ev_pending[2] = { false, false }; int flip = 0;
        hipKernelNodeParams pose_kp{};     // the pass-0 trace node as captured (grid, block, LDS) ...
        Params pose_P;                     // ... and the Params bytes it was captured with
    };
    std::vector<FrameGraph> graphs; int graph_gen = 0;
    DevBuf<float> d_poses;       // [RR_MAX_BATCH][8]: Params::pose_table, written by the pass-0 trace launch of every chain
    unsigned short last_rows[kMaxPasses] = {};     // rows the lane's last batch was launched with (0: the bound)

    // echo provenance (rr_labels.hip): per segment the list of tagged echoes [prov_seg][prov_cap] with its count, and the two label
    // columns [prov_seg][prov_cells].  Allocated by the lane's first provenance call (ensure_prov_buffers); plain batches never touch them
    DevBuf<EchoSrc> d_prov; DevBuf<uint32_t> d_prov_count, d_label_cols, d_face_cols;
    int prov_seg = 0, prov_cap = 0, prov_cells = 0;

    // wave paths (rr_paths.hip): k_wave_gather's running state per segment [path_seg], allocated by the lane's first paths call
    // (ensure_path_state)
    DevBuf<uint4> d_path_state; int path_seg = 0;

    // Doppler (rr_doppler.hip): k_rate_gather's state per wave and per segment, the rate list and the shifted list beside the lane's
    // echo lists, what the list-only column launch needs (a zero count for the last pass' slots, statistics of its own), the winner
    // columns; the call's sensor velocities and the twists on their way down (the host array stays alive with the lane, like the
    // beam tables above).  Allocated by the lane's first Doppler call (ensure_dop_buffers); plain batches never touch them
    DevBuf<float4> d_dop_state, d_dop_in; DevBuf<float2> d_dop_rate; DevBuf<SigRec> d_dop_sig; DevBuf<uint32_t> d_dop_count, d_dop_zero;
    DevBuf<SegStats> d_dop_stats; DevBuf<float> d_dop_vel_cols;
    std::vector<float4> h_dop_in;
    int dop_seg = 0, dop_cap = 0, dop_echo_cap = 0, dop_cells = 0; size_t dop_obj = 0;
    StagePool stage;              // the outputs of the host forms of rr_side.hip on their way to the host

    hipStream_t stream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_consumed = nullptr;
    bool pending_consume = false;
    // host delivery (rr_simulate_batch_host_async): TWO delivery slots per lane, used alternately, each an image buffer with its
    // event (behind the assemble that filled it; on the stream-ordered route behind the copy) and the copy that empties it.  A
    // slot is written again two uses of the lane later (eight batches with four lanes), by which time its copy has long left --
    // the host settles the slot before it reuses the buffer and practically never has to wait (with ONE buffer the SDMA route
    // waited for the lane's previous batch every time: the lane's stream ran dry while the host issued the next chain -- 35.9k
    // instead of 39.4k images/s on config 2 from a C++ caller, 2.5k instead of 4.3k with one pose per batch on the target).
    // Every other user of the lane settles both slots (take_lane); rr_simulate assembles its image in slot 0's buffer
    Delivery slot[2]; int next_slot = 0;
};

}  // namespace rr
using namespace rr;     // (an internal header: its includers are the library's own host files, which all work in rr)

struct rr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // scene
    bool have_mesh = false;
    // ONE allocation: the BVH4 nodes, then the leaf-order triangles -- child references are float4 offsets
    // from its base (rr_bvh.h), so a traversal step forms its address the same way for a node and a leaf
    DevBuf<float4> d_bvh;
    uint32_t tri_base4 = 0;        // float4 offset of triangle 0
    uint64_t n_nodes = 0, n_tris = 0;
    uint32_t depth = 0, stack_need = 0;
    float hit_pad = 0.f;           // grazing guard of the triangle test (leaf_step): 1e-5 x the extent of the faces' vertices = half the builders' box padding

    // dynamic scenes (rr_refit.hip): the rest geometry of the last rr_set_mesh* / rr_update_vertices, one rigid pose per
    // object; the traced scene is every face's rest corners moved by its object's pose
    DevBuf<float> d_rest_v, d_stage_v;     // [rest_nv][3]; the staging copy holds a new rr_update_vertices until it is validated
    DevBuf<uint32_t> d_rest_f;             // [rest_nf][3]
    size_t rest_nv = 0, rest_nf = 0;
    uint32_t n_objects = 1;
    std::vector<float> poses;              // [n_objects][7] qx qy qz qw tx ty tz
    DevBuf<float> d_poses, d_stage_poses;
    std::vector<float> twists;             // [n_objects][6] vx vy vz wx wy wz (rr_set_object_twists): by value, read only by the Doppler calls
    bool dyn_ready = false;                // the per-level node lists below belong to the current tree
    bool rebuilding = false;               // rr_rebuild_tree: the build it runs keeps the rest data
    DevBuf<uint32_t> d_levels;             // node indices, root level first
    std::vector<uint32_t> level_off;       // level d = [level_off[d], level_off[d + 1])
    bool cost_known = false; double cost_at_build = 0.0;    // SAH cost of the tree as built (first dynamic call on it)
    // what the builder knew: the nodes as built (copied before the first refit: a leaf of split parts keeps its clipped
    // box while its objects stay where they were), the poses the tree was built for, whether the rest vertices changed since
    DevBuf<float4> d_built; bool have_built = false; float built_hit_pad = 0.f;
    std::vector<float> build_poses; bool verts_dirty = false;
    DevBuf<uint8_t> d_moved;
    DevBuf<float> d_red; DevBuf<double> d_cost;              // per-workgroup partials of the two reductions

    // params
    rr_config cfg;
    bool have_cfg = false;
    std::vector<rr_material> materials;
    std::vector<int32_t> object_materials;
    int32_t material_id_air = 0;
    bool have_materials = false;
    std::vector<float> beams;   // xyz
    std::vector<float> noise;
    int noise_rows = 1;
    int motion_rows = 1;
    bool motion_live = false;    // a motion table was in use at the last upload (Params::motion_poses non-null)
    std::vector<float> motion;   // [n_angles][7] or empty
    std::vector<float> smear;
    int smear_mode = 0;

    DevBuf<float4> d_qas, d_beams, d_materials;
    DevBuf<double> d_mat_limits;   // [n_materials]: angle of total reflection per material
    double limit_same = 0.0;       // ... and for v2 = 0.3f (the same material on both sides): computed once, at rr_create
    DevBuf<uint32_t> d_beam_order, d_beam_order2;
    DevBuf<int32_t> d_objmat;
    DevBuf<float> d_smear, d_noise, d_motion, d_decay;
    // what upload_tables() has to refresh (the reference node re-reads its parameters before EVERY
    // frame, radar_simulator.cpp:85,200: setters that bring nothing new must cost nothing)
    enum : unsigned { D_CFG = 1, D_BEAMS = 2, D_MAT = 4, D_NOISE = 8, D_MOTION = 16, D_ALL = 31 };
    unsigned tables_dirty = D_ALL;

    // frame lanes: each owns a full set of frame buffers + a stream, so consecutive
    // frames overlap on the GPU (the tail of one frame's k_trace runs beside the next frame)
    std::vector<Lane> lanes;
    size_t next_lane = 0, last_lane = 0;
    size_t next_stream_lane = 0;
    int stream_lanes = 3;          // lanes whose own stream rr_simulate_device uses

    bool stats_mode = false;
    int pass0_az = 16;
    int stack_lds_max = 64;      // traversal stack entries kept in LDS (RR_STACK_LDS lowers it: tests of the spill path)
    int timing = 0;   // 0 off, 1 every kernel, 2 k_trace only
    std::map<std::string, KernelTimer> timers;
    // timing events are pooled: created once, handed out in the frame path, returned when rr_get_kernel_time
    // reads them (no hipEventCreate / hipEventDestroy between the synchronisation points of a timed region)
    std::vector<hipEvent_t> event_pool;
    hipEvent_t take_event() {
        if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
        hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
    }

    int passes_override = -1;    // a parameter batch in the making: the largest n_reflections of its sets sizes queues and launch loops
    // Scratch of the device forms, which run on arbitrary caller streams: one pool per stream a form has been called on, its slots shared by
    // every form (rr_stage.h: Scratch).  It lives with the context, is used on the caller's stream only -- calls on one stream are ordered by
    // that stream, calls on different streams may overlap on the GPU -- and grows only with that stream drained.  scratch_mu guards the map,
    // not the pools.  It is not staging and never aliases a host form's pool below: a host form holds slots of its stage while the device form
    // it calls takes scratch on the same stream
    std::map<hipStream_t, StagePool> scratch; std::mutex scratch_mu;
    StagePool& scratch_of(hipStream_t s) { std::lock_guard<std::mutex> lock(scratch_mu); return scratch[s]; }
    int metrics_hist = 0;        // RR_METRICS_HIST
    StagePool stage;             // the round trips of the host forms on c->stream (rr_images.hip, rr_sets.hip)
    void* h_rb = nullptr; size_t h_rb_bytes = 0;         // page-locked: read_back()
    void* h_frame = nullptr; size_t h_frame_bytes = 0;   // page-locked: error bits + per-pass counters of rr_simulate's frame

    bool roctx = false;
    int seg_chunk = 16;          // later-pass trace grids in chunks of S neighbouring segments, segment-fast inside a chunk (RR_TRACE_CHUNK; 0: rows of one segment)
    int stackless = 0;           // RR_STACKLESS=1: the stack-free traversal (no LDS; DESIGN.md §3 says what it costs)
    int cull_pop = 1;            // k_trace's later passes drop stack entries at pop time (RR_CULL_POP=0: off; the images are the same either way)
    // RR_HOST_SDMA (1): rr_simulate_batch_host_async hands a batch's images to ROCr's SDMA path (rr_sdma.cpp: one worker thread,
    // copies in order, each behind its batch's last kernel) instead of a copy the HIP runtime would pick an engine for; 0, a
    // pageable destination, statistics mode or a runtime ROCr cannot be reached through: a stream-ordered copy behind the batch
    // (copy_out)
    int host_sdma = 1; SdmaCopier* sdma = nullptr; bool sdma_tried = false;
    // rr_deliver_to_host_async: copies of caller-owned device buffers that rr_wait_host fences (no image buffer); events are pooled
    std::vector<Delivery> deliveries;
    std::vector<hipEvent_t> delivery_events;
    int tight_grid = 1;          // later-pass trace rows sized by what earlier batches needed (RR_TIGHT_GRID=0: the doubling bound)
    int tight_force = 0;         // RR_TIGHT_FORCE=n: rows of n workgroups whatever the history says (tests of the repair path)
    int hist_gen = 1;            // bumped whenever mesh / materials / beam / config change: the lanes' histories start over
    int use_graphs = 1;          // RR_GRAPHS=0: every launch chain is issued kernel by kernel
    int graph_gen = 1;           // bumped whenever anything a captured launch bakes in may have changed (tables, tree, lane buffers)
    uint64_t graph_clock = 0, graph_replays = 0, graph_captures = 0;
};

namespace rr {
// roctx ranges around the enqueue of trace / shade / scan / column / assemble (readable rocprofv3
// timelines with --marker-trace).  Optional: RR_ROCTX=1 loads librocprofiler-sdk-roctx / libroctx64 at run time (rr_create).
typedef int (*roctx_push_fn)(const char*);
typedef int (*roctx_pop_fn)(void);
inline roctx_push_fn g_roctx_push = nullptr; inline roctx_pop_fn g_roctx_pop = nullptr;
inline void roctx_push(const char* name) { if (g_roctx_push) g_roctx_push(name); }
inline void roctx_pop() { if (g_roctx_pop) g_roctx_pop(); }
int fail(rr_ctx* c, int code, const std::string& msg);      // (c == nullptr: the error of rr_create)

inline hipStream_t stream_of(const rr_ctx* c, void* stream) { return stream ? (hipStream_t)stream : c->stream; }

#define RR_HIP(c, expr)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((c), -100, std::string(#expr) + ": " + hipGetErrorString(e_));         \
    } while (0)

struct TimedScope {
    rr_ctx* c; hipStream_t s; const char* name; hipEvent_t a = nullptr, b = nullptr;
    bool on;
    TimedScope(rr_ctx* c_, hipStream_t s_, const char* n_) : c(c_), s(s_), name(n_) {
        on = c->timing == 1;
        if (on) { a = c->take_event(); b = c->take_event(); (void)hipEventRecord(a, s); }
        if (c->roctx) roctx_push(name);
    }
    ~TimedScope() {
        if (on) { (void)hipEventRecord(b, s); c->timers[name].pending.emplace_back(a, b); }
        if (c->roctx) roctx_pop();
    }
};

// timing mode 1, kernels of the frame chain: the launch's own begin / end timestamps (hipExtLaunchKernel events) -- a kernel's
// duration as rocprofv3 reports it, whatever it waited for before it started (TimedScope's stream events include that wait)
struct KernelEvents {
    rr_ctx* c; const char* name; hipEvent_t a = nullptr, b = nullptr;
    KernelEvents(rr_ctx* c_, const char* n_) : c(c_), name(n_) {
        if (c->timing == 1) { a = c->take_event(); b = c->take_event(); }
        if (c->roctx) roctx_push(name);
    }
    ~KernelEvents() {
        if (a) c->timers[name].pending.emplace_back(a, b);
        if (c->roctx) roctx_pop();
    }
};

// a parameter batch as run_frame sees it: per frame its passes and beam group, per group the frame pass 0 is traced for
struct SetPlan {
    int n_groups = 1;
    unsigned char frame_passes[64], frame_beam[64], group_frame[64];
    const float4* d_beams = nullptr; const uint32_t* d_order = nullptr; const uint32_t* d_order2 = nullptr;   // [n_groups][n_beam]; null: the ctx's tables
};

// what a call wants of run_frame beyond pose, azimuth block and stream
struct FrameJob {
    int n_frames = 1;
    uint8_t* d_cols_u8 = nullptr;        // the caller's column buffer; null: the lane's own
    float* d_cols_f32 = nullptr;         // ... and its f32 columns, or with lane_f32 the lane's own; neither: none
    bool lane_f32 = false;
    const float4* d_matsets = nullptr;   // a parameter batch: one material table per frame [n_frames][mat_stride], its plan (null: material
    int mat_stride = 0;                  // sets only: the context's beams, every frame the config's passes)
    const SetPlan* plan = nullptr;
    int provenance = 0;                  // 1: the lane's echo lists are gathered; 2: and its label columns made
    const WaveOut* paths = nullptr;      // the wave records of every pass go to these rows (state: the lane's, filled in by run_frame)
    const DopArgs* doppler = nullptr;    // gain and the caller's rows: a provenance chain whose image comes from the shifted list (the lane's buffers are filled in by run_frame)
    const float* sensor_vel = nullptr;   // ... and its sensor velocities [n_frames][3], or null: 0
};

// rr_api.hip
int check_ready(rr_ctx* c);
int upload_tables(rr_ctx* c);
void beam_trace_orders(const float* beams, size_t nb, std::vector<uint32_t>& order, std::vector<uint32_t>& order2);
int read_back(rr_ctx* c, void* dst, const void* d_src, size_t bytes);
int overflow_error(rr_ctx* c, uint32_t bits, bool since_sync = false);
// the counters of the lane the last frame ran on (the callers have synchronised)
inline int read_counters(rr_ctx* c, Counters& h) { return read_back(c, &h, c->lanes[c->last_lane].d_counters.p, sizeof(h)); }
// ... and its error bits as the failure of a synchronous call: reported here, so cleared from the lane's sticky word
inline int report_frame_errors(rr_ctx* c)
{
    Counters h;
    const int rc = read_counters(c, h); if (rc) return rc;
    if (h.overflow) RR_HIP(c, hipMemset(c->lanes[c->last_lane].d_sticky.p, 0, sizeof(uint32_t)));
    return overflow_error(c, h.overflow);
}

// rr_images.hip
int check_compare(rr_ctx* c, const char* who, const void* imgs, int n_images, const void* ref, uint32_t which, int win_size, const void* out,
                  const void* hist);      // the refusals of rr_compare_images* / rr_simulate_param_sets_metrics

// rr_frame.hip
void drop_graphs(Lane& L);
int prepare_lane(rr_ctx* c, Lane& L, int n_seg, bool want_f32 = false);
bool host_visible(const void* p);
int settle_lane(rr_ctx* c, Lane& L, int slot = -1, const void* only_dst = nullptr);
int take_lane(rr_ctx* c, size_t li, hipStream_t s, int slot = -1);
hipError_t give_lane(Lane& L, hipStream_t s);
int ensure_prov_buffers(rr_ctx* c, Lane& L);
// The launch chain of a batch on lane L, enqueued on s: `pose` [job.n_frames][7] (a parameter batch: one pose), azimuths [az_begin, az_end)
// of every frame.  A plain call leaves the job empty: one frame into the lane's own columns
int run_frame(rr_ctx* c, Lane& L, const float* pose, int az_begin, int az_end, hipStream_t s, const FrameJob& job = {});
int assemble_frames(rr_ctx* c, const Lane& L, uint8_t* dst, int n_frames, hipStream_t s);

}  // namespace rr
