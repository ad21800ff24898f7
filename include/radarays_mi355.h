/*
 * radarays_mi355.h -- C ABI of libradarays_mi355.so
 *
 * MI355X (gfx950) implementation of ONE path of uos/radarays_ros: the
 * per-azimuth multi-bounce radar ray loop of RadarCPU::simulate
 * (src/radarays_ros/RadarCPU.cpp:155-548), behind the reference's own seam
 *     virtual sensor_msgs::ImagePtr Radar::simulate(ros::Time)      (include/radarays_ros/Radar.hpp:64)
 * The reference has no FFI: backends are C++ subclasses of `Radar` chosen at
 * start-up (src/radar_simulator.cpp:118-176).  A third subclass `RadarHIP`
 *  marshals the protected state `simulate()` reads
 * (Radar.hpp:66-105) into the calls below -- plain pointers and sizes only.
 *
 * Threading: one rr_ctx is used by one thread at a time; one ctx per GPU.  Several GPUs of one node behind ONE
 * object: rr_multi (below) -- one process, one ctx per device, one RCCL collective per call.
 * Errors: every call returns 0 on success, <0 on error; rr_last_error() gives
 * the text.  No exceptions cross this boundary.  There is NO CPU fallback: if
 * no HIP device is usable rr_create() fails.
 */
#ifndef RADARAYS_MI355_H
#define RADARAYS_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_ABI_VERSION 7
#define RR_MAX_BATCH 64   /* frames (poses or material sets) one call renders in one set of launches */

typedef struct rr_ctx rr_ctx;

/* msg/RadarMaterial.msg:1-4 -- m_params.materials.data[] (Radar.hpp:84) */
typedef struct rr_material {
    float velocity;   /* m/ns; 0.3 = air; 0 = nothing is transmitted */
    float ambient;    /* A in  E * (A + B * cos(theta)^C)  (RadarCPU.cpp:310-316) */
    float diffuse;    /* B */
    float specular;   /* C */
} rr_material;

/* The RadarModelConfig fields (cfg/RadarModel.cfg:11-85) and RadarModel fields
 * (msg/RadarModel.msg:1-3) that RadarCPU::simulate reads, plus the constants
 * Radar::Radar fixes (src/radarays_ros/Radar.cpp:22-32). */
typedef struct rr_config {
    int32_t n_cells;                 /* RadarModel.cfg:16   rows of the polar image */
    int32_t n_angles;                /* Radar.cpp:29        400 azimuth columns */
    int32_t n_reflections;           /* RadarModel.cfg:29   number of ray-cast passes (RadarCPU.cpp:220) */
    int32_t signal_denoising;        /* RadarModel.cfg:44   0 none 1 triangular 2 gaussian 3 maxwell-boltzmann */
    int32_t signal_denoising_triangular_width;   /* :46 */
    int32_t signal_denoising_gaussian_width;     /* :48 */
    int32_t signal_denoising_mb_width;           /* :50 */
    int32_t ambient_noise;           /* RadarModel.cfg:60   0 none 1 uniform 2 perlin */
    int32_t scroll_image;            /* :81 */
    int32_t record_multi_reflection; /* :83 */
    int32_t record_multi_path;       /* :82 */
    int32_t max_waves_per_azimuth;   /* build's own: capacity of the per-azimuth wave queue per pass;
                                        0 = n_samples * 2^(n_reflections-1) clamped to 65536 */
    int32_t brdf_model;              /* build's own: 0 = the checkout's A + B cos^C (radar_algorithms.h:168-187);
                                        1 = Cook-Torrance lobe, A + B * D_GGX * G_Smith normalised to 1 at normal
                                        incidence, alpha^2 = 2 / (C + 2) (BASELINE.json configs[4]; the reference's own
                                        version lives on its dev/flex branch, outside the checkout: PARITY UNPINNED) */
    int32_t reserved_;
    double  resolution;              /* :15  m per range bin */
    double  energy_max;              /* :32 */
    double  signal_max;              /* :33 */
    double  signal_denoising_triangular_mode;    /* :47 */
    double  signal_denoising_gaussian_mode;      /* :49 */
    double  signal_denoising_mb_mode;            /* :51 */
    double  ambient_noise_at_signal_0;           /* :61 */
    double  ambient_noise_at_signal_1;           /* :62 */
    double  ambient_noise_energy_max;            /* :63 */
    double  ambient_noise_energy_min;            /* :64 */
    double  ambient_noise_energy_loss;           /* :65 */
    double  multipath_threshold;                 /* :84 */
    float   wave_energy_threshold;   /* Radar.cpp:24  0.001 */
    float   theta_min;               /* Radar.cpp:28  0 */
    float   theta_inc;               /* Radar.cpp:27  -(2 pi)/400 */
    float   range_max;               /* radar_algorithms.cpp:158  1000 (ray tfar) */
} rr_config;

/* Counters of the last simulated frame (optional; reading them synchronises). */
typedef struct rr_stats {
    uint64_t wave_passes;     /* waves ray-cast, all passes */
    uint64_t hits;
    uint64_t signals;
    uint64_t nodes_visited;   /* only counted when the ctx was put in stats mode */
    uint64_t tris_tested;
    uint32_t overflow;        /* 1: wave queue capacity exceeded (frame invalid) */
    uint32_t pad_;
} rr_stats;

/* Fills *cfg with the defaults of cfg/RadarModel.cfg + Radar.cpp:22-32. */
void rr_default_config(rr_config* cfg);

/* Context bound to HIP device `device` (what the RadarCPU/RadarGPU constructor
 * does with its map handle, RadarCPU.hpp:21-28).  NULL on failure. */
rr_ctx* rr_create(int device);
void    rr_destroy(rr_ctx* ctx);
const char* rr_last_error(const rr_ctx* ctx);   /* ctx may be NULL: create error */
int     rr_abi_version(void);

/* Replaces rm::import_embree_map (src/radar_simulator.cpp:149): triangle soup
 * + per-face object id (index into object_materials; NULL -> all 0).  Builds
 * the BVH on the host (SAH over references with spatial splits: a face larger than its neighbours may be cut and
 * then has one triangle record per leaf that holds a part of it) and uploads it.  For meshes of up to 2M triangles
 * the tree is CHOSEN by measurement: the plain SAH tree (no spatial splits) is built as well, both trace the same sample
 * of radar-like rays on the GPU, the one with fewer traversal steps stays (RR_BVH_CHOOSE).  Inputs are copied.  Size limit:
 * 8 x BVH4 nodes + 3 x triangle records < 2^28 (child references are 28-bit offsets), i.e. about 50M triangles; a
 * mesh whose split parts would exceed it is built without spatial splits. */
int rr_set_mesh(rr_ctx* ctx, const float* verts /*[nv][3]*/, size_t nv,
                const uint32_t* faces /*[nf][3]*/, size_t nf,
                const uint32_t* face_object_id /*[nf] or NULL*/);

/* Same contract, but the BVH is built ON THE GPU (early split clipping of oversized faces + Morton codes + rocprim
 * radix sort + Karras radix tree + refit + 4-wide collapse): 0.35 s instead of 1.9 s for 10M triangles, tree of
 * lower quality (rays traverse about 1.2x slower than through the host builder's SAH tree with spatial splits).
 * Images are bit-identical whichever builder made the tree: the nearest hit is defined independently of
 * traversal order. */
int rr_set_mesh_gpu(rr_ctx* ctx, const float* verts /*[nv][3]*/, size_t nv,
                    const uint32_t* faces /*[nf][3]*/, size_t nf,
                    const uint32_t* face_object_id /*[nf] or NULL*/);

/* The finished tree of `src` (either builder), copied device to device into `ctx` -- `ctx` may sit on another GPU
 * (hipMemcpyPeer over xGMI) or on the same one.  What rr_multi_set_mesh uses to replicate the map after ONE build
 * (radar_simulator.cpp:149 loads the map once per process).  Both contexts are drained first; `src` keeps its tree.
 * The rest geometry and the object poses (dynamic scenes, below) are copied too: the copy can be posed on its own. */
int rr_copy_mesh(rr_ctx* ctx, rr_ctx* src);

/* ---- dynamic scenes: per-object rigid poses, the tree refit in place ----
 * A context with a mesh holds REST GEOMETRY -- the vertices and faces last given to rr_set_mesh, rr_set_mesh_gpu or
 * rr_update_vertices, kept on the device (12 B per vertex + 12 B per face: about 180 MB at 10M triangles; an
 * rr_update_vertices keeps a second vertex copy while it validates; the first dynamic call on a tree also keeps a copy of
 * its nodes as built, 128 B per node) -- and ONE RIGID POSE PER OBJECT.  Objects are numbered
 * as in face_object_id: n_objects = max(face_object_id) + 1, or 1 when the ids are NULL.  After rr_set_mesh* every pose is
 * the identity.
 * The traced scene is always face f's three rest corners moved by pose[object(f)].  A pose is float[7] = qx qy qz qw
 * tx ty tz (the sensor pose's layout); moving a point is p' = q_rot(q, p) + t in f32 with rr_device.h's q_rot term order,
 * not fused; the quaternion is used as given (not normalised); a pose equal to (0,0,0,1,0,0,0) is applied as a plain copy.
 * Contract: after any of the calls below every image, hit and count equals what a fresh rr_set_mesh of the POSED TRIANGLE
 * SOUP renders (the moved corners, same face order, same object ids), up to the grazing residual class DESIGN.md §2.2 states
 * for spatially split trees -- a refit tree holds whole-triangle boxes, so it is closer to brute force than a fresh split
 * tree is.  The tree keeps its topology; its boxes are recomputed level by level (rr_refit.hip), so traversal slows as
 * objects travel far from where the tree was built: rr_get_tree_cost says when rr_rebuild_tree pays.  Objects still at
 * their as-built pose keep the builder's clipped leaf boxes; after rr_update_vertices every leaf bounds whole triangles
 * until the next rebuild (slow on maps whose large faces the host builder split: DESIGN.md §11).
 * Each call drains the work in flight on the context first (as rr_set_mesh does) and returns when the tree is updated:
 * batches submitted earlier render the old scene, later ones the new.  A refused call (< 0, rr_last_error: wrong count,
 * non-finite value -- a pose, or a posed corner -- or no mesh) leaves the scene untouched.  A refit whose posed extent is
 * unchanged keeps the captured launch graphs (the grazing guard's hit_pad is the only value they bake in that a refit can
 * change); the traversal stack bound depends on the topology only. */
int rr_set_object_poses(rr_ctx* ctx, const float* poses /*[n][7]*/, size_t n);        /* n == n_objects */
int rr_update_vertices(rr_ctx* ctx, const float* verts /*[nv][3]*/, size_t nv);       /* nv == rest nv: new rest geometry, poses kept */
/* One TWIST PER OBJECT for the Doppler calls (below): float[6] = vx vy vz wx wy wz, map frame, m/s and rad/s, taken about the map
 * origin: a point p of object b moves with v_b(p) = V_b + Omega_b x p (f32, the cross product in rr_device.h's v_cross term order, not
 * fused).  n == n_objects, or 0: every twist back to zero; they are also zero after rr_set_mesh* / rr_copy_mesh.  The twists are
 * stored by value and read only by the Doppler calls: nothing is drained, the tree and the launch graphs are not touched, and no
 * other call renders differently.  Refused with the twists untouched: -2 without a mesh, -3 for a wrong count, a null array or a
 * non-finite value. */
int rr_set_object_twists(rr_ctx* ctx, const float* twists /*[n][6]*/, size_t n);
/* SAH-style cost of the current boxes (sum over child records of half-area / the root's half-area, weighted 1 per inner
 * child and `count` per leaf child) and of the tree as built (measured at the first dynamic call on the tree) */
int rr_get_tree_cost(rr_ctx* ctx, double* cost_now, double* cost_at_build);
/* a fresh tree of the posed scene with builder 0 (host SAH, as rr_set_mesh) or 1 (GPU LBVH, as rr_set_mesh_gpu); the rest
 * geometry and the poses stay */
int rr_rebuild_tree(rr_ctx* ctx, int builder);

/* Radar::loadParams (Radar.cpp:220-226): materials, object_materials,
 * material_id_air. */
int rr_set_materials(rr_ctx* ctx, const rr_material* materials, size_t n_materials,
                     const int32_t* object_materials, size_t n_objects,
                     int32_t material_id_air);

/* Radar::updateDynCfg (Radar.cpp:188-218). */
int rr_set_config(rr_ctx* ctx, const rr_config* cfg);

/* m_waves_start (RadarCPU.cpp:136-145): beam sample directions in the local
 * azimuth frame, as sample_cone_local (radar_algorithms.cpp:248-294) returns
 * them.  The reference draws them from std::random_device, so they are an
 * input here. */
int rr_set_beam_samples(rr_ctx* ctx, const float* dirs /*[n][3]*/, size_t n);

/* per-azimuth `random_begin` of the ambient-noise stage (RadarCPU.cpp:472);
 * [n_angles].  Needed only when ambient_noise != 0.  The reference draws fresh offsets for every frame
 * (RadarCPU.cpp:461-472): a caller of the single-frame entry points sets a new row before each frame; for
 * the batch entry points n may be k * n_angles (k >= 2 rows), frame f of a batch then uses row f % k. */
int rr_set_noise_offsets(rr_ctx* ctx, const float* rnd, size_t n);

/* include_motion = true (RadarCPU.cpp:190-196, cfg/RadarModel.cfg:85 -- the .cfg default): the reference looks
 * Tsm up once PER AZIMUTH.  poses = [n_angles][7] (qx,qy,qz,qw,tx,ty,tz); while set, every
 * rr_simulate* call uses poses[azimuth] and ignores its own pose argument (which must still
 * be a valid pose).  n = 0 switches back to one pose per frame.  For the batch entry points n may be
 * k * n_angles (k tables, one sweep of the antenna each): frame f of a batch then uses table f % k, like the
 * rows of rr_set_noise_offsets -- the reference's default mode through the batched / multi-GPU path.  A pose batch of
 * more than one frame while exactly ONE table is set is refused (-3): every frame would be the same sweep and the call's
 * poses would be ignored silently.  (A parameter batch renders every set with table 0.) */
int rr_set_motion_poses(rr_ctx* ctx, const float* poses, size_t n);

/* RadarCPU::simulate for azimuths [az_begin, az_end) with sensor pose
 * Tsm = {quaternion x,y,z,w ; translation x,y,z} (Radar::updateTsm,
 * Radar.cpp:80-132).  Host buffers, synchronous:
 *   out_u8  [n_cells][n_angles] row-major, step n_angles  == the mono8
 *           sensor_msgs::Image of RadarCPU.cpp:555-561; only the columns of
 *           the simulated azimuths are written.
 *   out_f32 optional, same layout: the float slice before convertTo(CV_8U).
 *   stats   optional. */
int rr_simulate(rr_ctx* ctx, const float pose_qxyzw_t[7], int az_begin, int az_end,
                uint8_t* out_u8, float* out_f32, rr_stats* stats);

/* Same, asynchronous on `stream` (a hipStream_t; NULL = the ctx's own stream)
 * with DEVICE buffers.  d_cols_u8 receives the simulated columns column-major:
 * [az_end-az_begin][n_cells] (this is the block a rank contributes to the
 * multi-GPU gather).  d_cols_f32 optional, same layout. */
int rr_simulate_columns_device(rr_ctx* ctx, const float pose_qxyzw_t[7], int az_begin, int az_end,
                               uint8_t* d_cols_u8, float* d_cols_f32, void* stream);

/* Frame batch (multi-GPU weak scaling, offline generation): the same azimuth block
 * [az_begin, az_end) of n_frames (1..RR_MAX_BATCH) different poses in ONE set of launches.
 * poses = [n_frames][7]; d_cols_u8 = [n_frames][az_end-az_begin][n_cells].  Kernels then see
 * n_frames x block segments, i.e. a rank that owns 1/N of the azimuths of N frames does the
 * same amount of work per launch as a single GPU does for one whole frame. */
int rr_simulate_batch_columns_device(rr_ctx* ctx, const float* poses, int n_frames, int az_begin, int az_end,
                                     uint8_t* d_cols_u8, void* stream);

/* Whole frames of n_frames (1..RR_MAX_BATCH) poses in one set of launches, everything on `stream` (no internal
 * streams: callers that want several batches in flight issue them on several streams, 4 is the measured
 * optimum): d_imgs_u8 = [n_frames][n_cells][n_angles].  The throughput entry point for offline generation
 * from C/C++ (tools/cpp_bench.cpp: 41k images/s at config 2 with 4 poses per call on 4 streams). */
int rr_simulate_batch_device(rr_ctx* ctx, const float* poses, int n_frames, uint8_t* d_imgs_u8, void* stream);

/* The reference leaves every frame in HOST memory (m_polar_image -> sensor_msgs::Image, RadarCPU.cpp:542,555-561).
 * Whole frames of n_frames poses like rr_simulate_batch_device, delivered to the caller's host buffer
 * h_imgs_u8 = [n_frames][n_cells][n_angles].  Returns at once; the images are COMPLETE ONLY after rr_wait_host(ctx,
 * h_imgs_u8) (NULL: every outstanding buffer) or rr_synchronize() -- until then the buffer must stay valid and must not be
 * read.  How the bytes travel is the library's business.  By default they leave at once over the SDMA engines, submitted
 * through ROCr by worker threads of the context behind the batch's last kernel (csrc/rr_sdma.cpp; two image buffers per
 * frame lane, so the host does not wait for a copy before it issues the lane's next batch): no shader core stores a byte of
 * them, and it is the same engine whichever HIP runtime serves the process (a ROCm 7.0.2 runtime, e.g. the one a Python ML
 * wheel bundles, would carry a hipMemcpyAsync as a blit kernel: 27-35k images/s on config 2 where SDMA delivers the link's
 * 39k).  Where that path is not available (RR_HOST_SDMA=0, a pageable buffer, statistics mode, no reachable ROCr) the
 * images leave on a plain copy behind the batch, on `stream` (rr_copy_to_host_async's route: about 7 % fewer images/s than
 * SDMA on the target, where the copy's PCIe-paced stores hold up the stores of the kernels beside it).  Issue batches on
 * up to four streams (HIP maps streams onto four hardware queues) and hand the buffers out from a ring twice as deep as
 * the batches in flight.  h_imgs_u8 should be page-locked (rr_host_alloc / rr_host_free = hipHostMalloc); a pageable
 * buffer works through the plain copy.  rr_destroy drops images that nobody waited for.  "Returns at once" has two
 * exceptions: a lane whose two previous deliveries are both still in flight makes the call wait for the older one, and
 * so does a buffer reallocation. */
int rr_simulate_batch_host_async(rr_ctx* ctx, const float* poses, int n_frames, uint8_t* h_imgs_u8, void* stream);
int rr_wait_host(rr_ctx* ctx, const void* h_imgs_u8);
void* rr_host_alloc(size_t bytes);
void  rr_host_free(void* p);

/* bytes of device memory -> host memory, asynchronous on `stream`, by the library's own copy kernel (8 workgroups of 256
 * threads on one XCD, 16 B per thread and store) when h_dst is page-locked and both pointers
 * and the size are multiples of 16 -- else a plain hipMemcpyAsync.  Why an entry point: which engine carries a
 * hipMemcpyAsync to page-locked memory is the choice of the HIP runtime in the caller's process (a ROCm 7.0.2 runtime
 * launches a blit kernel per copy and reads 27-36k images/s on config 2, the image's own ROCm 7.2 uses SDMA: 39.4k);
 * the library's deliveries that must be STREAM-ordered take this route (the fallback copies of rr_simulate_batch_host_async
 * where SDMA is not available); measured, a shader-core copy is no faster than the runtime's blit kernel (24-31k on config 2)
 * -- callers that can fence with rr_wait_host use rr_deliver_to_host_async below.  Replaces nothing in the reference
 * (cv_bridge deep-copies m_polar_image on the host, RadarCPU.cpp:555-558). */
int rr_copy_to_host_async(rr_ctx* ctx, const void* d_src, void* h_dst, size_t bytes, void* stream);
/* The same for a caller that can fence with rr_wait_host instead of the stream: bytes of a caller-owned device buffer leave
 * over the SDMA engines (the route of rr_simulate_batch_host_async, csrc/rr_sdma.cpp) once the work enqueued on `stream` so
 * far has completed.  Returns at once; h_dst is complete -- and d_src may be overwritten -- after rr_wait_host(ctx, h_dst)
 * (NULL: everything outstanding) or rr_synchronize().  Where the SDMA path is not available it is rr_copy_to_host_async plus
 * an event.  rr_multi's root and the sharded step loop (radarays_ros_amd/dist.py) deliver this way. */
int rr_deliver_to_host_async(rr_ctx* ctx, const void* d_src, void* h_dst, size_t bytes, void* stream);
/* Which route the host deliveries of this context take: 2 = SDMA through ROCr (csrc/rr_sdma.cpp) is in use; 1 = it will be
 * tried by the first delivery; 0 = a stream-ordered copy behind the batch (RR_HOST_SDMA=0, or the path was not available /
 * was switched off -- RR_HOST_SDMA_VERBOSE=1 says why).  bench.py prints it on its line, the GPU tests assert it. */
int rr_host_delivery_route(rr_ctx* ctx);

/* Assemble the mono8 image from column-major columns, applying scroll_image
 * (RadarCPU.cpp:457): d_img[c][(scroll + a) % n_angles] = d_cols[a][c].
 * Device buffers, asynchronous on `stream`. */
int rr_assemble_image_device(rr_ctx* ctx, const uint8_t* d_cols_u8 /*[n_angles][n_cells]*/,
                             uint8_t* d_img_u8 /*[n_cells][n_angles]*/, void* stream);

/* Same for columns that arrive in blocks of n_loc azimuths `block_stride` BYTES apart (what a rank
 * holds after the all_to_all of a multi-frame step: [source rank][frame][n_loc][n_cells]):
 * azimuth a is read at d_cols + (a / n_loc) * block_stride + (a % n_loc) * n_cells. */
int rr_assemble_blocks_device(rr_ctx* ctx, const uint8_t* d_cols_u8, int n_loc, size_t block_stride,
                              uint8_t* d_img_u8, void* stream);

/* Parameter batch: n_sets (1..RR_MAX_BATCH) material tables, ONE pose -> n_sets images.
 * Replaces n_sets round trips of the reference's optimisation loop, where every objective
 * evaluation sends one RadarParams goal to the gen_radar_image action and waits for one image
 * (action/GenRadarImage.action, scripts/radaray_opti.py:170-200; the server side sets
 * m_params.materials and calls simulate(), Radar.hpp:52-53).  `sets` is [n_sets][n_materials]
 * with n_materials as given to rr_set_materials (object -> material map, air id, config and beam
 * samples stay as set).  Pass 0 does not depend on the materials and is traced once for all sets;
 * image k is bit-identical to rr_set_materials(sets[k]) + rr_simulate_device(pose).
 * d_imgs_u8: [n_sets][n_cells][n_angles] in HBM, stream-ordered like rr_simulate_device. */
int rr_simulate_material_sets_device(rr_ctx* ctx, const float pose[7], const rr_material* sets, int n_sets,
                                     size_t n_materials /* per set; must equal rr_set_materials' count */,
                                     uint8_t* d_imgs_u8, void* stream);
/* Same with a host output buffer (synchronous). */
int rr_simulate_material_sets(rr_ctx* ctx, const float pose[7], const rr_material* sets, int n_sets,
                              size_t n_materials, uint8_t* out_imgs_u8);

/* The whole parameter vector of the optimiser (scripts/radaray_opti.py:36-113: beam_width, n_reflections, 2 x 4 material
 * values) batched the same way: set k = {material table, beam sample directions, number of ray-cast passes}, ONE pose,
 * n_sets (1..RR_MAX_BATCH) images in one set of launches.
 *   materials      [n_materials] (as many as rr_set_materials got), or NULL: the table of rr_set_materials
 *   beam_dirs      [n_beam][3] with n_beam as given to rr_set_beam_samples (what sample_cone_local returns for this set's
 *                  beam_width: rr_sample_cone_local), or NULL: the samples of rr_set_beam_samples.  Sets with the SAME
 *                  directions (same pointer or same bytes) form a group: pass 0 does not depend on the materials and is
 *                  traced once per group
 *   n_reflections  0..16 passes for this set, negative: the config's.  A set with fewer passes than the others simply
 *                  stops early (no live waves in the later launches); wave queues are sized for the largest
 * Image k is bit-identical to rr_set_materials / rr_set_beam_samples / rr_set_config(n_reflections) of set k followed
 * by rr_simulate_device(pose); every set sees the same noise realisation (row 0 of rr_set_noise_offsets).  One
 * difference in ERROR behaviour: with max_waves_per_azimuth left at 0 the queues of a batch are sized for its largest
 * number of passes (and a lane that already holds larger ones is reused as it is), so a set that alone would have run
 * into the 65,536-wave clamp of its own nominal capacity (n_samples x 2^(passes-1) beyond 65,536) may render completely
 * here where the one-by-one call returns -7; a user-set max_waves_per_azimuth is honoured exactly. */
typedef struct rr_param_set {
    const rr_material* materials;
    const float* beam_dirs;
    int32_t n_reflections;
    int32_t reserved_;
} rr_param_set;
int rr_simulate_param_sets_device(rr_ctx* ctx, const float pose[7], const rr_param_set* sets, int n_sets, size_t n_materials,
                                  uint8_t* d_imgs_u8 /* [n_sets][n_cells][n_angles] in HBM */, void* stream);
/* The objective of that optimiser is ONE float per evaluation -- minus the PSNR of the simulated image against one real
 * radar image (radaray_opti.py:170-211, skimage.metrics.peak_signal_noise_ratio on mono8) -- so an evaluation need not
 * ship 1.37 MB per set to the host: rr_score_images_device returns, for n images in HBM against one reference image in
 * HBM, psnr[k] = 10 log10(255^2 / mean((img_k - ref)^2)) in f64 (+inf for identical images; the device part is the
 * exact integer sum of squared differences, optionally returned in out_sse) to HOST arrays; synchronous on `stream`. */
int rr_score_images_device(rr_ctx* ctx, const uint8_t* d_imgs_u8, int n_images, const uint8_t* d_ref_u8,
                           double* out_psnr /* host [n_images], or NULL */, uint64_t* out_sse /* host [n_images], or NULL */, void* stream);
/* Host-buffer form (synchronous) of the parameter batch: out_imgs_u8 [n_sets][n_cells][n_angles] or NULL; with
 * ref_img_u8 (host, [n_cells][n_angles]) and out_psnr ([n_sets]) the scores come back as well -- with out_imgs_u8 NULL
 * an evaluation of n_sets parameter vectors returns n_sets doubles and no image leaves the GPU. */
int rr_simulate_param_sets(rr_ctx* ctx, const float pose[7], const rr_param_set* sets, int n_sets, size_t n_materials,
                           uint8_t* out_imgs_u8, const uint8_t* ref_img_u8, double* out_psnr);

/* ---- real-to-sim image metrics (rr_metrics.hip) -------------------------------------------------------------------
 * The reference's calibration loop imports five metrics (scripts/radaray_opti.py: structural_similarity,
 * peak_signal_noise_ratio, normalized_mutual_information, variation_of_information, mutual_info_score) and its evaluation
 * launch file publishes a "real to sim gap" between /Navtech/Polar and /radar/image (launch/tests/eval_real_to_sim.launch).
 * rr_compare_images_device computes all of them for n mono8 images in HBM against ONE reference image in HBM; one
 * rr_image_metrics record per image comes back to the host.  Images are uint8 [n_cells][n_angles] in the context's current
 * shape, N = n_cells * n_angles.
 *   PSNR / SSE (RR_METRIC_PSNR): exactly what rr_score_images_device returns (the same bits).
 *   SSIM (RR_METRIC_SSIM): skimage.metrics.structural_similarity on uint8 with its defaults -- a uniform w x w window
 *     (w = win_size, odd, 3..15; skimage's default is 7), K1 = 0.01, K2 = 0.03, data_range = 255 (C1 = (K1 * 255)^2,
 *     C2 = (K2 * 255)^2), sample covariance (cov_norm = w^2 / (w^2 - 1)); with ux, uy, uxx, uyy, uxy the window means of x, y,
 *     x^2, y^2, xy:  vx = cov_norm (uxx - ux^2), vy likewise, vxy = cov_norm (uxy - ux uy),
 *     S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)), and ssim = the mean of S over the pixels whose whole
 *     window lies inside the image (skimage's crop by (w - 1) / 2: no border rule is needed).  THE AZIMUTH AXIS IS NOT
 *     WRAPPED: columns 0 and n_angles - 1 are not neighbours here, as they are not in skimage.  The five window sums are
 *     exact integers, S and its mean are f64 in a fixed order.  win_size is read only with RR_METRIC_SSIM; an image smaller
 *     than the window in either direction is refused (-3).
 *   Joint histogram (RR_METRIC_INFO): H[a][b] = the number of pixels with image value a and reference value b, 256 x 256,
 *     exact uint32.  In nats, f64, skipping empty bins:  hxy = ln N - (1/N) sum c ln c over the joint counts -- summed as
 *     (1/N) sum c (ln N - ln c), the same number, which is exactly 0 when one bin holds every pixel -- and hx, hy the same
 *     over the marginals of the image (a) and of the reference (b);
 *     mi = hx + hy - hxy   (sklearn.metrics.mutual_info_score of the flattened images)
 *     nmi = (hx + hy) / hxy  (skimage's normalized_mutual_information at one bin per grey level); hxy == 0 -- both images
 *           constant, where skimage returns NaN -- gives nmi = 1
 *     voi = 2 hxy - hx - hy  (the sum of skimage's two variation_of_information terms)
 * `which` is a mask of RR_METRIC_* bits; the fields of a metric not asked for are 0.  d_joint_hist (HBM, uint32
 * [n_images][256][256], or NULL) receives the histograms; it needs RR_METRIC_INFO.  Synchronous on `stream` like
 * rr_score_images_device, and like it the call uses context-owned scratch (at most 64 images' histograms, 16 MB: more images
 * are worked through in chunks), one set per stream the call has been made on.  The device forms of this header that keep scratch in
 * the context share that set: it grows to the largest request a stream has seen, growing it drains that stream, and it is freed with
 * the context; a form called on a further stream costs one more set.  A config is needed, a mesh is not.
 * Refused with a message and nothing written: -2 without a config; -3 for a null buffer, n_images outside 1..65535, which == 0
 * or with unknown bits, an even or out-of-range win_size, an image smaller than the window, d_joint_hist without
 * RR_METRIC_INFO. */
#define RR_METRIC_PSNR 1u
#define RR_METRIC_SSIM 2u
#define RR_METRIC_INFO 4u
typedef struct rr_image_metrics {
    double psnr; uint64_t sse;
    double ssim;
    double hx, hy, hxy, mi, nmi, voi;
} rr_image_metrics;
int rr_compare_images_device(rr_ctx* ctx, const uint8_t* d_imgs_u8, int n_images, const uint8_t* d_ref_u8, uint32_t which,
                             int win_size, rr_image_metrics* out /* host [n_images] */,
                             uint32_t* d_joint_hist /* HBM [n_images][256][256], or NULL */, void* stream);
/* The host-buffer form, for real images from a bag: imgs_u8 [n_images][n_cells][n_angles], ref_u8 [n_cells][n_angles],
 * joint_hist host [n_images][256][256] or NULL.  Synchronous.  The images are staged 64 at a time; the records are written
 * once all of them are done, the histograms chunk by chunk (a refusal writes nothing; a device error, -100, in a later
 * chunk leaves `out` untouched and joint_hist with the chunks before it). */
int rr_compare_images(rr_ctx* ctx, const uint8_t* imgs_u8, int n_images, const uint8_t* ref_u8, uint32_t which, int win_size,
                      rr_image_metrics* out, uint32_t* joint_hist);
/* rr_simulate_param_sets with any of the metrics as the objective: out [n_sets] records of the simulated images against
 * ref_img_u8 (host, [n_cells][n_angles]); out_imgs_u8 (host) or NULL, and with NULL no image leaves the GPU. */
int rr_simulate_param_sets_metrics(rr_ctx* ctx, const float pose[7], const rr_param_set* sets, int n_sets, size_t n_materials,
                                   uint8_t* out_imgs_u8, const uint8_t* ref_img_u8, uint32_t which, int win_size,
                                   rr_image_metrics* out);

/* ---- azimuth registration (rr_align.hip) --------------------------------------------------------------------------
 * The metrics above compare at ONE azimuth alignment, but a real sweep and a simulated one do not start at the same azimuth
 * (hence scroll_image: azimuth k is written to column (scroll_image + k) % n_angles), and a change of sensor yaw is, to first
 * order, a circular shift along the azimuth axis.  Under such a shift the sums of x, x^2, r, r^2 do not change, so the cross
 * term alone gives the exact SSE, PSNR and normalised cross-correlation at EVERY shift.  The reference has no registration
 * step: this is the build's own definition.
 * Images are uint8 [n_cells][n_angles] in the context's current shape.  A cell window [cell_begin, cell_end) selects the rows
 * that take part (a real image has a bright near-field ring a caller wants to leave out); N = (cell_end - cell_begin) * n_angles.
 * For image x and reference r, and s in 0..n_angles-1:
 *   xcorr[s] = sum over c in the window and a of x[c][a] * r[c][(a + s) mod n_angles]        exact int64
 *            = sum(np.roll(x, s, axis=1) * r)
 *   s is the amount to ADD TO scroll_image so that x lines up with r.
 * With the exact integers Sx, Sxx, Sr, Srr (sums of x, x^2, r, r^2 over the window):
 *   sse[s]  = Sxx + Srr - 2 xcorr[s]                                                         exact uint64
 *   psnr    = from sse and N with the expression of rr_score_images_device (+inf at sse == 0)
 *   ncc[s]  = (N xcorr[s] - Sx Sr) / sqrt((N Sxx - Sx^2)(N Srr - Sr^2)): the numerator and the two factors are exact int64,
 *             converted to f64, then one multiply, one sqrt, one divide; 0 when either factor is 0
 *   shift   = the smallest s that attains max xcorr (also the minimum SSE and the maximum ncc: everything else is
 *             shift-invariant); n_best = the number of shifts that attain it
 * A record holds xcorr, sse, psnr and ncc AT `shift`; d_xcorr (HBM, int64 [n_images][n_angles], or NULL) receives the whole
 * curve.  Synchronous on `stream`, context-owned scratch, one set per stream the call has been made on, more than 64 images in
 * chunks: the conventions of rr_compare_images_device.  A config is needed, a mesh is not (rr_simulate_batch_align needs what
 * rr_simulate_batch_device needs).
 * Refused with a message and nothing written: -2 without a config; -3 for a null buffer, n_images outside 1..65535, a window
 * that is empty or outside 0..n_cells, a window of more than 2^23 pixels (which keeps N xcorr inside int64). */
typedef struct rr_align_record {
    int32_t shift, n_best;
    int64_t xcorr;            /* at `shift` */
    uint64_t sse; double psnr, ncc;   /* at `shift` */
    uint64_t sum_x, sum_xx, sum_r, sum_rr;   /* over the window */
} rr_align_record;
int rr_align_images_device(rr_ctx* ctx, const uint8_t* d_imgs_u8, int n_images, const uint8_t* d_ref_u8, int cell_begin, int cell_end,
                           rr_align_record* out /* host [n_images] */, int64_t* d_xcorr /* HBM [n_images][n_angles], or NULL */,
                           void* stream);
/* The host-buffer form: imgs_u8 [n_images][n_cells][n_angles], ref_u8 [n_cells][n_angles], xcorr host [n_images][n_angles] or
 * NULL.  Synchronous; staged 64 images at a time, the records written once all of them are done, the curves chunk by chunk. */
int rr_align_images(rr_ctx* ctx, const uint8_t* imgs_u8, int n_images, const uint8_t* ref_u8, int cell_begin, int cell_end,
                    rr_align_record* out, int64_t* xcorr);
/* rr_simulate_batch_device into a context-owned image buffer, then rr_align_images_device against ref_img_u8 (host,
 * [n_cells][n_angles]): n candidate poses x all n_angles yaws from n simulated images.  n_frames is 1..RR_MAX_BATCH;
 * out_imgs_u8 (host) or NULL, and with NULL no image leaves the GPU; xcorr host [n_frames][n_angles] or NULL. */
int rr_simulate_batch_align(rr_ctx* ctx, const float* poses, int n_frames, const uint8_t* ref_img_u8, int cell_begin, int cell_end,
                            uint8_t* out_imgs_u8, rr_align_record* out, int64_t* xcorr);

/* All frames of a multi-frame step in ONE launch: frame j reads its columns frame_stride bytes after
 * frame j-1 (block addressing as above) and writes image j of d_imgs_u8 [n_frames][n_cells][n_angles]. */
int rr_assemble_frames_device(rr_ctx* ctx, const uint8_t* d_cols_u8, int n_loc, size_t block_stride,
                              int n_frames, size_t frame_stride, uint8_t* d_imgs_u8, void* stream);

/* Convenience: rr_simulate_columns_device for all azimuths into the ctx's own
 * column buffer + rr_assemble_image_device into d_img_u8.  Asynchronous. */
int rr_simulate_device(rr_ctx* ctx, const float pose_qxyzw_t[7], uint8_t* d_img_u8, void* stream);

/* Blocks until `stream` (NULL = ctx stream) and the ctx's own frame lanes -- and, because batches may
 * have been issued on further caller streams, everything else on the device -- are idle, then reports what
 * the asynchronous (*_device) entry points could not: -7 if any frame enqueued since the last call
 * exceeded its wave/signal queue capacity, -8 if one met an object/material id outside the tables
 * (such a frame is truncated; the synchronous rr_simulate returns the same codes itself). */
int rr_synchronize(rr_ctx* ctx, void* stream);

/* Pipelined callers that must not drain the device to learn about an error: enqueues on `stream` (the one the LAST
 * *_device / *_host_async call ran on) a 4-byte copy of the error bits of the frame lane that call used (bit 0: wave /
 * signal queue overflow, bit 1: object / material id outside the tables; accumulated since the last rr_synchronize, which
 * reports and clears them) into *h_bits.  h_bits should be page-locked (rr_host_alloc); it is valid once `stream` has
 * reached this point.  rr_multi uses it per batch. */
int rr_peek_error_bits_async(rr_ctx* ctx, uint32_t* h_bits, void* stream);

/* Counters of the last frame (synchronises the ctx stream). */
int rr_get_stats(rr_ctx* ctx, rr_stats* stats);

/* stats mode: traversal counters (nodes_visited, tris_tested) on/off; off by
 * default because the counting kernel variant is slower. */
int rr_set_stats_mode(rr_ctx* ctx, int enable);
/* stats mode only: the wave-level shape of the traversal loop over the last frame (all k_trace launches), what
 * separates the kernel's instruction ISSUE rate from useful work (bench.py: roofline.useful_issue_frac).  A wave holds
 * 16 rays (one per quad of lanes) and iterates until its slowest ray is done; an iteration issues the node path if any
 * quad holds a node and the leaf path if any holds a leaf.
 *   out[0] waves   out[1] wave iterations   out[2] iterations that issued the node path   out[3] ... the leaf path
 *   out[4] live quad-steps (ray steps that did work; 16 x out[1] were issued)   out[5] longest wave (iterations)
 *   out[6] node steps of all rays (= nodes_visited)   out[7] leaf steps of all rays (= out[4] - out[6]) */
int rr_get_traversal_shape(rr_ctx* ctx, uint64_t out[8]);

/* ---- introspection used by tests / bench ---- */
/* nearest-hit query for rays given in map coordinates (device traversal). */
int rr_debug_trace(rr_ctx* ctx, const float* origs /*[n][3]*/, const float* dirs /*[n][3]*/, size_t n,
                   float* out_t /*[n], <0 = miss*/, uint32_t* out_face /*[n]*/);
/* BVH facts: nodes, leaf triangle records (>= faces: the host builder may cut a face by spatial splits and keeps
 * one record per part, at most twice the faces), depth, stack entries needed. */
/* Test hook: the kernels' own Fresnel split (k_shade's fresnel_split = radar_algorithms.h:55-139; the incidence angle by acosf of
 * the f32 dot product as k_shade forms it, the angle of total reflection by the function that fills the material table) on n
 * independent inputs: v1 = the wave's velocity (0.3 in the frame path, RadarCPU.cpp:107-110), v2 = the material's.  Host arrays
 * in, host arrays out; tests compare them with the oracle on the reference-derived cases of tests/golden/pyref_dense_*. */
int rr_debug_fresnel(rr_ctx* ctx, size_t n, const float* normals /*[n][3]*/, const float* dirs /*[n][3]*/, const double* energy /*[n]*/,
                     const double* v1 /*[n]*/, const float* v2 /*[n]*/,
                     float* out_refl_dir /*[n][3]*/, double* out_refl_energy /*[n]*/, float* out_refr_dir /*[n][3]*/, double* out_refr_energy /*[n]*/);
/* Test hook: the kernels' own back_reflection_shader (radar_algorithms.h:168-187 as RadarCPU.cpp:310-316,347-353 call it) on n
 * independent inputs, in5 = [n][5] (incidence angle, energy, ambient, diffuse, specular); brdf_model as in rr_config.  Tests compare
 * it with the oracle on the cases of tests/golden/pyref_brdf.npy (outputs of the reference's scripts/radarays_snell_fresnel_brdf.py). */
int rr_debug_brdf(rr_ctx* ctx, size_t n, const float* in5 /*[n][5]*/, int brdf_model, float* out /*[n]*/);
/* Test hook: k_column -- one azimuth's ordered echoes -> its range-bin column (RadarCPU.cpp:402-542) -- on echo streams given by
 * the caller, through the launcher the frame path uses (so a launch of >= 1024 segments runs the 256-thread form, a smaller one
 * the 512-thread form).  Needs rr_set_config only (no mesh): the denoiser, noise mode, scroll, n_cells, n_angles and the scale
 * factors are the config's, the noise offsets rr_set_noise_offsets'.  The streams of n_seg = n_frames * n_loc segments (segment
 * s = frame s / n_loc, azimuth az_begin + s % n_loc) go into the buffers of one frame lane, sized as for a frame by the
 * config and rr_set_beam_samples (wave capacity: max_waves_per_azimuth or n_samples * 2^(n_reflections - 1); signal capacity:
 * the sum of the passes' wave bounds, twice that with record_multi_path), in the two forms the kernel reads:
 *   list  [n_seg][list_stride], list_count [n_seg]: the compacted echoes of passes 0 .. n_passes - 2 (read when n_passes > 1)
 *   slots [n_seg][2 * slot_stride]: the last pass' per-wave slots, wave j = records 2j (path echo) and 2j + 1 (multipath echo),
 *         cell < 0 = empty; slot_hit [n_seg][slot_stride]: wave j hit; slot_count [n_seg]: waves of the last pass (n_passes > 1;
 *         with n_passes == 1 every segment has n_beam).  Without record_multi_path the kernel stages the even records only.
 * An echo with cell >= n_cells is dropped by the kernel like an empty one.  Out: out_u8 [n_seg][n_cells], out_f32 the same or NULL,
 * out_stats [n_seg][3] = the last pass' wave_passes, hits, signals, or NULL.  -3 (nothing written) for anything the lane's buffers
 * cannot hold: n_passes > max(1, n_reflections), n_beam or slot_stride above the wave capacity, list_stride above the signal
 * capacity, a count above its stride, an azimuth block outside the image.  Tests compare it with the oracle's column step. */
typedef struct rr_echo { int32_t cell; float strength; } rr_echo;
int rr_debug_column(rr_ctx* ctx, int n_frames, int n_loc, int az_begin, int n_passes, int n_beam, int record_multi_path,
                    const rr_echo* list, const uint32_t* list_count, size_t list_stride,
                    const rr_echo* slots, const uint8_t* slot_hit, const uint32_t* slot_count, size_t slot_stride,
                    float* out_f32, uint8_t* out_u8, uint32_t* out_stats /*[n_seg][3]*/);
int rr_get_bvh_info(rr_ctx* ctx, uint64_t* n_nodes, uint64_t* n_tris, uint32_t* depth, uint32_t* stack_need);
/* How the later-pass trace launches are sized (round 5).  A segment holds at most n_beam * 2^pass waves in pass `pass`;
 * instead of a row of 16-ray workgroups up to that bound per segment, a row is as long as earlier batches of this context
 * needed (the largest per-segment count seen per pass, + 1/16 + 32 rays), and a segment that exceeds its row anyway is
 * finished by a small repair launch -- images never depend on the history.  Synchronises the device.
 *   out_rows[p]  workgroups per segment row of pass p in the last call's launches (0: the doubling bound)
 *   out_hist[p]  the largest per-segment wave count seen in pass p since mesh / materials / beam / config last changed
 *   *repaired_groups  16-ray groups the repair launches had to trace since then (0 once the history has settled) */
int rr_get_trace_grid(rr_ctx* ctx, uint32_t out_rows[24], uint32_t out_hist[24], uint64_t* repaired_groups);
/* Launch graphs (round 5): the launch chain of a pose batch (rr_simulate_batch_*_device, rr_simulate_columns_device,
 * rr_multi's device entries) that has been issued before with the same shape -- azimuth block, frames, output buffer,
 * trace rows -- is captured in a hipGraph on its second use and replayed from then on: one hipGraphLaunch instead of
 * 4..20 kernel launches (host time per chain 46 -> ~11 us at 4 passes); the poses of a replay travel as the parameters of the
 * graph's first node.  Parameter batches and instrumented runs (timing / statistics / roctx) are issued kernel by
 * kernel.  Any setter, mesh change or buffer reallocation drops the captured graphs.
 * Returns how many chains this context has captured / replayed. */
int rr_get_graph_stats(rr_ctx* ctx, uint64_t* captures, uint64_t* replays);
/* average duration (ms) of the trace kernel launches since the last call with
 * reset!=0, measured with hipEvents on the launch stream when timing mode is
 * on; also returns the number of launches.  Used by bench.py for roofline. */
int rr_set_timing_mode(rr_ctx* ctx, int enable /* 0 off, 1 every kernel, 2 k_trace only */);
int rr_get_kernel_time(rr_ctx* ctx, const char* kernel /* "trace0"|"trace"|"trace_repair"|"shade"|"scan"|"column"|"assemble"|"gather"|"label";
                                                            "trace" = the later-pass launches WITHOUT the k_trace_repair launch that
                                                            follows a tightened row, which is "trace_repair" */,
                       double* total_ms, uint64_t* launches, int reset);

/* every launch duration (ms) recorded for `kernel` since the last reset ("trace0" = pass 0, "trace" = later
 * passes, ...): *n_out = count, the first min(count, capacity) values go to out_ms (may be NULL). */
int rr_get_kernel_samples(rr_ctx* ctx, const char* kernel, float* out_ms, size_t capacity, size_t* n_out);
/* pre-creates n timing events so that a timed region never calls hipEventCreate */
int rr_reserve_timing_events(rr_ctx* ctx, size_t n);

/* ---- echo provenance: per-echo face, object and pass; label images (rr_labels.hip) ------------------------------
 * What a pixel is made of: which triangle and object produced a return, in which ray-cast pass (pass > 0: a multi-bounce
 * ghost), and whether it is a multipath echo.  An opt-in variant of the pose-batch frame call returns, beside the usual image,
 *   the echo stream: per azimuth the ordered list of echoes exactly as the column step consumes it (the reference's order: passes
 *                    in sequence, waves in order, a wave's path echo before its multipath echo), every echo with the face it came
 *                    from, that face's object id, the pass and the kind.  Echoes whose cell lies beyond the image are listed too
 *                    (the column step drops them); echoes that were pruned or never emitted have no record
 *   label images   : per pixel of the polar image the echo that contributes the largest single term to that range bin.
 * info word of an echo = object id (bits 0..23) | pass << 24 (4 bits) | kind << 28 (0: path echo, 1: multipath echo); top bits 0.
 * A ghost mask is `pass > 0`, a semantic mask is object -> material on the host.
 * Definition of a label.  The reference has no such output: parity is UNPINNED and this is the build's own definition (a numpy
 * restatement in tests/labels_ref.py checks the kernel bit for bit).  For one azimuth with ordered echoes e_0 .. e_{n-1}; W, mode
 * and the f32 weights w[0..W) are exactly what the column step uses (signal_denoising == 0: W = 1, mode = 0, w[0] = 1):
 *   echo k reaches bin g iff 0 <= cell_k < n_cells, 0 < g < n_cells and 0 <= g - (cell_k - mode) < W; bin 0 is never written
 *        (RadarCPU.cpp:424)
 *   its term is v = (float)((double)strength_k * (double)w[g - cell_k + mode]): the product is exact in f64, then one rounding
 *   only a finite v > 0 takes part
 *   the winner of bin g is the largest key (bits(v) << 32) | (0xFFFFFFFF - k): equal terms go to the echo that comes first
 *   label[g] = info_k and face[g] = face_k of the winner; a bin nobody reaches gets RR_LABEL_NONE in both planes
 * Ambient noise, energy_max and the final scale play no part: a labelled bin may still render 0, and a noisy bin may have no label.
 * Limits.  n_cells <= RR_LABEL_MAX_CELLS (the label column is held as 64-bit keys in LDS: 64 KB; rr_set_config admits no more).  The info word holds object ids
 * below 2^24 - 1 and passes below 16: a call on a mesh with 2^24 - 1 or more objects or a config with n_reflections > 16 (which
 * rr_set_config does not admit either) is refused (-3).  Pose batches only: parameter batches share the hits of pass 0 between frames.  rr_set_motion_poses and
 * rr_set_noise_offsets apply as in rr_simulate_batch_device.  The chain of a provenance call is issued kernel by kernel (never
 * from a launch graph), the image is made by the same launches with the same arguments as rr_simulate_batch_device's: the same
 * bytes.  The lane's provenance buffers (n_angles x n_frames lists of 16-byte records, two uint32 columns) are allocated by the
 * first provenance call; plain batches never touch them.
 * Refused with a message and nothing written: -2 without a config / mesh / materials / beam where the frame calls refuse, -3 for a
 * null required buffer, n_frames outside 1..RR_MAX_BATCH, d_echoes without d_echo_counts, echo_stride == 0 with d_echoes,
 * n_cells > RR_LABEL_MAX_CELLS, the object / pass limits above; rr_debug_labels also for a count above its stride. */
typedef struct rr_echo_src { int32_t cell; float strength; uint32_t face; uint32_t info; } rr_echo_src;   /* 16 B */
#define RR_LABEL_NONE 0xFFFFFFFFu
#define RR_LABEL_MAX_CELLS 8192
/* whole frames of n_frames (1..RR_MAX_BATCH) poses, asynchronous on `stream`, device buffers:
 *   d_imgs_u8   [n][n_cells][n_angles]                      as rr_simulate_batch_device, same bytes
 *   d_labels    uint32 [n][n_cells][n_angles] or NULL       info of the winning echo, image layout (scroll applied)
 *   d_faces     uint32 [n][n_cells][n_angles] or NULL
 *   d_echoes    rr_echo_src [n][n_angles][echo_stride] or NULL, indexed by AZIMUTH (not column), in the reference's order
 *   d_echo_counts uint32 [n][n_angles] (required with d_echoes): the TRUE count; when it exceeds echo_stride the first
 *               echo_stride echoes are written and nothing beyond them (the convention of rr_detect_device's offsets) */
int rr_simulate_batch_provenance_device(rr_ctx* ctx, const float* poses, int n_frames, uint8_t* d_imgs_u8,
                                        uint32_t* d_labels, uint32_t* d_faces, rr_echo_src* d_echoes, size_t echo_stride,
                                        uint32_t* d_echo_counts, void* stream);
/* one frame, host buffers, synchronous; any output may be NULL except out_u8 (out_echoes needs out_echo_counts).  Returns -7 / -8
 * itself like rr_simulate. */
int rr_simulate_provenance(rr_ctx* ctx, const float pose[7], uint8_t* out_u8, uint32_t* out_labels, uint32_t* out_faces,
                           rr_echo_src* out_echoes, size_t echo_stride, uint32_t* out_echo_counts);
/* Test hook, config only (no mesh), like rr_debug_column: the label kernel on caller-given streams of n_seg segments (segment s =
 * azimuth az_begin + s; 1 <= n_seg, az_begin + n_seg <= n_angles), host arrays: echoes [n_seg][stride], counts [n_seg]; out columns
 * [n_seg][n_cells], not assembled.  Denoiser and n_cells are the config's. */
int rr_debug_labels(rr_ctx* ctx, int n_seg, int az_begin, const rr_echo_src* echoes, const uint32_t* counts, size_t stride,
                    uint32_t* out_labels, uint32_t* out_faces);

/* ---- wave paths: every wave's ray, hit, parent and echo per azimuth (rr_paths.hip) -------------------------------
 * By which route a return got there: the reference answers it with its inspection tool src/ray_reflection_test.cpp (shoot rays,
 * follow the reflect / refract bounces, draw the paths).  An opt-in variant of the pose-batch frame call returns, beside the usual
 * image, the wave list of every azimuth: one 64-byte record per wave that was RAY-CAST, misses included -- so the length of an
 * azimuth's list is its share of rr_stats.wave_passes.  The definition is the build's own (the reference keeps no such list);
 * it is pinned to the reference through the per-hit functions and the echo log of the oracle (tests/paths_ref.py restates the
 * bounce loop of one azimuth from them).
 * Order.  Passes in sequence; inside a pass the reference's order: the position j in the pass' live list, in pass 0 the beam index
 * j.  A wave at position k of pass p + 1 sits in child slot s of pass p: its parent is position s >> 1 of pass p and its branch
 * 1 + (s & 1) (1: reflection child, 2: transmission child; 0: an emitted beam).
 * Frame.  o and d are in the azimuth's SENSOR frame, bit for bit what the wave queue holds (pass 0: o = 0, d = the beam
 * direction); with RR_WAVES_MAP_FRAME they are q_am * o + t_am and q_am * d of the azimuth's sensor-to-map transform -- the
 * expressions the ray-cast sets its ray up with (pass 0: o = t_am).  energy and time do not depend on the frame.  The hit
 * point is o + range * d, formed by the caller.
 * Echo index.  `echo` counts in the azimuth's echo stream as rr_simulate_batch_provenance_device returns it for the same pose:
 * echoes of earlier passes + the echoes of the waves before this one in its pass.  The stream's record at that index has this
 * wave's face, object and pass.
 * Limits: pose batches only (-3 otherwise: parameter batches share the hits of pass 0); the object / pass limits of the
 * provenance info word; n_frames in 1..RR_MAX_BATCH.  The chain of a paths call is issued kernel by kernel (never from a launch
 * graph, and the lane's launch graphs are left alone); the image is made by the same launches with the same arguments as
 * rr_simulate_batch_device's: the same bytes.  The records go straight into the caller's rows; the lane keeps 16 bytes of
 * running state per segment, allocated by the first paths call.  rr_multi has no paths call: use the context of one device.
 * Refused with a message and nothing written: -2 without a config / mesh / materials / beam, -3 for a null required buffer
 * (poses, image, d_waves without d_wave_counts), wave_stride == 0 with d_waves, n_frames out of range, unknown flag bits, the
 * object / pass limits. */
typedef struct rr_wave_rec {          /* 64 B, four 16-B stores */
    float    o[3];  float range;      /* start point; hit distance along d, -1.0f for a miss */
    float    d[3];  uint32_t face;    /* direction; face id of the triangle hit, RR_LABEL_NONE for a miss */
    double   energy, time;            /* at the START of the wave (pass 0: 1.0, 0.0; RadarCPU.cpp:107,112) */
    uint32_t info;                    /* object id of the face (0xFFFFFF for a miss) | pass << 24 | branch << 28 | has_path_echo << 30 |
                                         has_multipath_echo << 31 */
    int32_t  parent;                  /* index of the parent wave in THIS azimuth's list; -1 in pass 0 */
    uint32_t material;                /* the medium the wave travels in (pass 0: 0, RadarCPU.cpp:111) */
    int32_t  echo;                    /* index of the wave's first echo in this azimuth's echo stream; -1 if none.  A wave with both
                                         echoes owns echo and echo + 1 (path echo first) */
} rr_wave_rec;
#define RR_WAVES_MAP_FRAME 1u         /* flags: o / d in the map frame */
#define RR_WAVES_MAX_PASSES 16        /* row length of d_pass_counts (n_reflections <= 16, as the info word demands) */
/* whole frames of n_frames poses, asynchronous on `stream`, device buffers:
 *   d_imgs_u8     [n][n_cells][n_angles]                       as rr_simulate_batch_device, same bytes
 *   d_waves       rr_wave_rec [n][n_angles][wave_stride] or NULL (16-byte aligned), indexed by AZIMUTH (not column)
 *   d_wave_counts uint32 [n][n_angles] or NULL (required with d_waves): the TRUE count; when it exceeds wave_stride the first wave_stride records
 *                 are written and nothing beyond them; parent and echo stay true indices even when their target was cut off
 *   d_pass_counts uint32 [n][n_angles][RR_WAVES_MAX_PASSES] or NULL: waves cast per pass (0 beyond n_reflections) */
int rr_simulate_batch_paths_device(rr_ctx* ctx, const float* poses, int n_frames, uint8_t* d_imgs_u8, rr_wave_rec* d_waves,
                                   size_t wave_stride, uint32_t* d_wave_counts, uint32_t* d_pass_counts, unsigned flags, void* stream);
/* one frame, host buffers, synchronous; out_waves and out_pass_counts may be NULL.  Returns -7 / -8 itself like rr_simulate. */
int rr_simulate_paths(rr_ctx* ctx, const float pose[7], uint8_t* out_u8, rr_wave_rec* out_waves, size_t wave_stride,
                      uint32_t* out_wave_counts, uint32_t* out_pass_counts, unsigned flags);

/* ---- Doppler: per-echo range rate and the FMCW range shift it causes (rr_doppler.hip) ------------------------------
 * An FMCW sweep turns a target's range rate into a range offset, dr = kappa * v_r (kappa set by the chirp): the Doppler distortion
 * of Navtech data (MulRan, Boreas, Oxford), next to the motion distortion of include_motion.  An opt-in variant of the pose-batch
 * frame call renders the image from the SHIFTED echo stream and returns the range rate and the shifted cell of every echo.  The
 * reference has no such output and renders every scene as if it stood still: parity is UNPINNED and this is the build's own
 * definition (a numpy restatement in tests/doppler_ref.py checks the kernels bit for bit).
 * Range rate of an echo.  For the echo of wave k of one azimuth follow `parent` (wave paths, above) back to the beam: the chain
 * w_0 .. w_k.  Geometry in the map frame exactly as RR_WAVES_MAP_FRAME records it: u_i the direction of w_i, p_i = o_i + range_i * u_i
 * its hit point, b_i the object of its face, v_i = v_{b_i}(p_i) (rr_set_object_twists), v_s the sensor's linear velocity in the map
 * frame (the antenna origin is the pose's translation, so the antenna's spin moves no origin), t_am the azimuth's sensor origin.  The
 * one-way path length is L = sum range_i; to first order (Fermat: a specular point sliding along its surface does not change L)
 *     dL/dt = -(v_s . u_0) + sum_{i<k} v_i . (u_i - u_{i+1}) + v_k . u_k
 *   path echo (kind 0)     : returns along the same path (time_back = 2 t): v_r = dL/dt
 *   multipath echo (kind 1): returns straight to the sensor (RadarCPU.cpp:325-360): v_r = 0.5 * (dL/dt + (v_k - v_s) . e),
 *                            e = normalize(p_k - t_am)
 * Positive v_r: receding.  All f32, not fused; the sum is accumulated in the order written, from the beam to the echo; each
 * difference u_i - u_{i+1} is formed before its dot product; dot products in rr_device.h's v_dot term order; normalize is
 * v_normalize.  Transmission branches use the geometric length (the reference's waves all travel at 0.3 m/ns).
 * Shifted cell.  `gain` is kappa in seconds (metres of range per m/s), finite, its sign the chirp direction.  With the echo's time as
 * the chain forms it (RadarCPU.cpp:410-413: half_time = (float)(time / 2), signal_dist = (float)(0.3 * (double)half_time)):
 *     r' = signal_dist + gain * v_r            (one f32 multiply, one f32 add, not fused)
 *     cell' = (int)((double)r' / resolution)   when that quotient is finite and lies in [0, 2^31); otherwise the echo is dropped
 * With gain == 0, or with every velocity zero, cell' is the chain's cell bit for bit.  Strength is unchanged.
 * Outputs of rr_simulate_batch_doppler_device (device buffers, asynchronous on `stream`):
 *   d_imgs_u8     [n][n_cells][n_angles]           the image the column step makes from the shifted stream (a list-only stream, the form
 *                                                  rr_debug_column shows); denoiser, ambient noise, energy_max, scale and scroll as
 *                                                  rr_simulate_batch_device
 *   d_echo_vel    float [n][n_angles][echo_stride] or NULL: v_r of every echo
 *   d_echo_cells  int32 [n][n_angles][echo_stride] or NULL: cell' of every echo, -1 for a dropped one
 *                 both indexed exactly like the echo stream of rr_simulate_batch_provenance_device for the same pose: by AZIMUTH, in
 *                 the reference's order, echoes beyond the image listed
 *   d_echo_counts uint32 [n][n_angles] or NULL (required with either row buffer): the TRUE count; when it exceeds echo_stride the
 *                 first echo_stride echoes are written and nothing beyond them
 *   d_vel_img     float [n][n_cells][n_angles] or NULL: per pixel (image layout, scroll applied) the v_r of the echo that wins the bin
 *                 by the label definition above (largest single term, ties to the earlier echo) applied to the shifted cells; NaN for
 *                 a bin nobody reaches.  Needs n_cells <= RR_LABEL_MAX_CELLS
 *   sensor_vel    float [n][3] per frame, or NULL: 0
 * Pose batches only; rr_set_motion_poses (each azimuth its own t_am) and rr_set_noise_offsets apply as in the plain batch.  The chain
 * is issued kernel by kernel, never from a launch graph, and the lane's launch graphs are left alone.  The lane's Doppler buffers (32
 * bytes per wave and pass parity, 16 bytes per echo) are allocated by the first Doppler call; plain batches never touch them.
 * rr_multi has no Doppler call: use the context of one device.
 * Refused with a message and nothing written: -2 without a config / mesh / materials / beam; -3 for a null required buffer (poses,
 * image, a row buffer without d_echo_counts), echo_stride == 0 with a row buffer, n_frames outside 1..RR_MAX_BATCH, a non-finite
 * gain or sensor velocity, n_cells > RR_LABEL_MAX_CELLS with d_vel_img, the object / pass limits of the provenance info word. */
int rr_simulate_batch_doppler_device(rr_ctx* ctx, const float* poses, int n_frames, const float* sensor_vel /*[n][3] or NULL = 0*/,
                                     float gain, uint8_t* d_imgs_u8, float* d_echo_vel, size_t echo_stride, uint32_t* d_echo_counts,
                                     int32_t* d_echo_cells, float* d_vel_img, void* stream);
/* one frame, host buffers, synchronous; any output may be NULL except out_u8 (a row buffer needs out_echo_counts); out_f32 as
 * rr_simulate's.  Returns -7 / -8 itself like rr_simulate. */
int rr_simulate_doppler(rr_ctx* ctx, const float pose[7], const float sensor_vel[3], float gain, uint8_t* out_u8, float* out_f32,
                        float* out_echo_vel, size_t echo_stride, uint32_t* out_echo_counts, int32_t* out_echo_cells, float* out_vel_img);

/* ---- radar point clouds and Cartesian images from polar images (rr_detect.hip) ----------------------------------
 * The reference's pipeline turns every simulated image into a point cloud with radar_tools/radar_img_to_pcl
 * (launch/tests/radar_sim_test.launch:80-84), a node outside the checkout: its algorithm is unknown, so parity with it is
 * UNPINNED and the two detectors below are this build's own, stated exactly (a numpy restatement in tests/detect_ref.py
 * checks them bit for bit).  Any context with a config converts images (a mesh is not needed: real MulRan / Navtech polar
 * images go through the same calls).  The images are [n_frames][n_cells][n_angles] u8 in the context's current shape;
 * geometry and config are read BY VALUE when the call is made (a later rr_set_config does not touch an enqueued call).
 *   image column col holds azimuth a = (col - scroll_image) mod n_angles   (the inverse of the assemble, RadarCPU.cpp:457)
 *   bin b lies at range r = (float)(((double)b + 0.5) * resolution)       (the bin centre of RadarCPU.cpp:521)
 *   azimuth a points along yaw theta = theta_min + (float)a * theta_inc  (RadarCPU.cpp:202), so a point is
 *   (x, y, z) = r * (cosf(theta), sinf(theta), 0) in the sensor frame of its own azimuth (no de-skew).
 * A refused call (-3: a config field outside its range, n_frames outside 1..65535, a null buffer, max_points < 0) writes
 * nothing; -2 without a config.  The device forms run on `stream` (NULL: the ctx's stream), write nothing but the caller's
 * buffers and use no context-owned memory, so they may run on any stream beside batches in flight.  The host forms stage
 * the images into context-owned buffers and are synchronous. */
typedef struct rr_detect_config {
    int32_t method;         /* 0 = CA-CFAR along range, 1 = k-strongest per azimuth */
    int32_t guard_cells;    /* CA-CFAR: G cells skipped on each side of the cell under test, 0..1024 */
    int32_t train_cells;    /* CA-CFAR: T training cells on each side, 1..1024 */
    int32_t k;              /* k-strongest: detections per azimuth, 1..n_cells */
    int32_t min_intensity;  /* 0..255: a cell below it is never a detection (both methods) */
    int32_t min_bin;        /* 0..n_cells-1: bins below it are never detections (near-field / leakage) */
    float   cfar_scale;     /* CA-CFAR threshold factor, finite, >= 0 */
    int32_t reserved_;
} rr_detect_config;

typedef struct rr_radar_point {  /* 24 B; x,y,z + intensity = geometry_msgs/Point32 + one ChannelFloat32 */
    float    x, y, z;       /* metres, sensor frame of that azimuth */
    float    intensity;     /* the cell's u8 value */
    uint32_t column;        /* image column */
    uint32_t bin;           /* range bin (image row) */
} rr_radar_point;

typedef struct rr_cartesian_config {
    int32_t width;          /* output is width x width pixels, 1..8192 */
    int32_t interpolation;  /* 0 = nearest, 1 = bilinear */
    float   pixel_size;     /* metres per pixel, finite, > 0 */
    int32_t reserved_;
} rr_cartesian_config;

/* method 0 (CA-CFAR), guard_cells 2, train_cells 16, k 12, min_intensity 1 (an empty cell is never a detection), min_bin 0,
 * cfar_scale 3.0 */
void rr_default_detect_config(rr_detect_config* cfg);

/* Detection, per column z[0..N) of every frame (N = n_cells):
 * CA-CFAR (method 0): every bin i >= min_bin is tested; its training cells are [i-G-T, i-G-1] and [i+G+1, i+G+T] clipped to
 *   [0, N) (cells below min_bin train too), n = their count, S = their uint32 sum; i is a detection iff z[i] >= min_intensity,
 *   n > 0 and (float)(z[i] * n) > cfar_scale * (float)S  (exact integers in f32 and one rounded f32 multiply).
 * k-strongest (method 1): the candidates are the bins i >= min_bin with z[i] >= min_intensity; the k largest are kept (value
 *   descending, then bin ascending); a column with fewer candidates keeps all of them.
 * Output: within a frame, points sorted by column ascending, then bin ascending, at d_points + f * max_points.
 *   d_offsets[f][c] = the number of detections in columns 0..c-1 (exclusive prefix), so d_offsets[f][n_angles] is the frame's
 *   TRUE total, also when it exceeds max_points: then the first max_points points in that order are written and nothing
 *   beyond them.  max_points == 0 (d_points may be NULL) counts only. */
int rr_detect_device(rr_ctx* ctx, const uint8_t* d_imgs_u8 /*[n][n_cells][n_angles]*/, int n_frames,
                     const rr_detect_config* cfg, rr_radar_point* d_points /*[n][max_points] or NULL if max_points==0*/,
                     int max_points, uint32_t* d_offsets /*[n][n_angles+1]*/, void* stream);
int rr_detect(rr_ctx* ctx, const uint8_t* imgs_u8, int n_frames, const rr_detect_config* cfg,
              rr_radar_point* points, int max_points, uint32_t* offsets);        /* host buffers, synchronous */

/* Windowed CFAR (rr_window.hip): a training window over range AND azimuth, and an ordered-statistic threshold, beside the two
 * detectors above.  The build's own definition like them (tests/window_ref.py restates it with loops and sorted()); the image is
 * z[b][col], N = n_cells bins by A = n_angles columns in the context's current shape. */
typedef struct rr_window_detect_config {
    int32_t method;          /* 0 CA, 1 GO, 2 SO, 3 OS */
    int32_t guard_range;     /* Gr 0..1024 */
    int32_t train_range;     /* Tr 0..1024 */
    int32_t guard_azimuth;   /* Ga 0..32 */
    int32_t train_azimuth;   /* Ta 0..32 */
    int32_t rank_permille;   /* OS: 1..1000 */
    int32_t min_intensity;   /* 0..255 */
    int32_t min_bin;         /* 0..n_cells-1 */
    float   scale;           /* finite, >= 0 */
    int32_t reserved_[3];
} rr_window_detect_config;

/* method 3 (OS), guard_range 2, train_range 16, guard_azimuth 1, train_azimuth 2, rank_permille 750, min_intensity 1, min_bin 0,
 * scale 3.0 */
void rr_default_window_detect_config(rr_window_detect_config* cfg);

/* Training cells of the cell under test (i, c): the cells (b, c') with |b - i| <= Gr + Tr and |c' - c| <= Ga + Ta (column distance
 *   on the circle) minus the guard box |b - i| <= Gr, |c' - c| <= Ga.  Rows are clipped to [0, N); columns wrap mod A (the scroll is
 *   a rotation of columns, so wrapping columns is wrapping azimuths); cells below min_bin train too.  n = their count, S = their sum.
 * Refused with -3, nothing written: a field outside its range, Tr + Ta == 0, 2 (Ga + Ta) + 1 > A, an unclipped window
 *   (2 (Gr + Tr) + 1) (2 (Ga + Ta) + 1) of more than 65,535 cells (so 255 * n < 2^24: every product below is an exact f32 integer),
 *   method 1 or 2 with Tr == 0, and whatever rr_detect refuses of frames and buffers.
 * Candidates: bins i >= min_bin with z >= min_intensity and n > 0.
 * CA (0): a detection iff (float)(z * n) > scale * (float)S.  With Ga = Ta = 0 this is rr_detect's method 0.
 * GO (1) / SO (2): the near half is the training cells of rows < i, the far half those of rows > i (training cells of row i belong
 *   to neither).  The means are compared exactly, S_near * n_far against S_far * n_near in uint64: GO takes the half with the
 *   greater mean, SO the smaller, ties go to near; if one half is empty both take the other, if both are there is no detection.
 *   Then the CA test with that half's (n_h, S_h).
 * OS (3): r = max(1, (n * rank_permille + 999) / 1000), v = the r-th smallest training value (1-based); a detection iff
 *   (float)z > scale * (float)v.
 * Output: points, order, d_offsets, truncation and max_points == 0 exactly as rr_detect_device; the geometry is rr_detect's.
 *   d_mask (or NULL): uint8 [n][N][A], 255 at a detection and 0 elsewhere, written whole; it goes into rr_label_components as it is.
 * The device form reads config and geometry by value, touches no context memory and needs no room but the caller's buffers (a count
 * pass, the scan of rr_detect, an emit pass), so it may run on any stream beside batches in flight. */
int rr_detect_window_device(rr_ctx* ctx, const uint8_t* d_imgs_u8 /*[n][n_cells][n_angles]*/, int n_frames,
                            const rr_window_detect_config* cfg, rr_radar_point* d_points /*[n][max_points] or NULL if max_points==0*/,
                            int max_points, uint32_t* d_offsets /*[n][n_angles+1]*/, uint8_t* d_mask /*[n][n_cells][n_angles] or NULL*/,
                            void* stream);
int rr_detect_window(rr_ctx* ctx, const uint8_t* imgs_u8, int n_frames, const rr_window_detect_config* cfg,
                     rr_radar_point* points, int max_points, uint32_t* offsets, uint8_t* mask);   /* host buffers, synchronous */
/* The tile a launch uses for this config and shape: out = (rows, columns, halo rows, halo columns).  A workgroup owns `columns`
 * adjacent columns of a frame and walks down them `rows` bins at a time, staging each step with Gr + Tr halo rows above and below
 * and Ga + Ta wrapped halo columns left and right.  `columns` shrinks as n_cells grows (16 up to 1024 bins, 8 up to 2048, 4 beyond),
 * so the workgroup count grows with n_cells.  The tile depends on the config and the shape alone: a base that is not 16-byte aligned
 * (or n_angles % 16 != 0) changes how a step is loaded (bytes, not 16-byte words from the multiple of 16 at or below the halo), not
 * the tile.  0, or -3 for a config or shape the detector refuses. */
int rr_detect_window_tile_sizes(const rr_window_detect_config* cfg, int n_cells, int n_angles, int out[4]);

/* Cartesian bird's-eye image, all in f32 with no fused operations.  c = (width - 1) * 0.5f; pixel (row i, col j) sits at
 * x = (c - i) * pixel_size (forward = up), y = (c - j) * pixel_size (left = left); rho = sqrtf(x*x + y*y), phi = atan2f(y, x).
 *   u = (phi - theta_min) / theta_inc, then u = fmodf(u, n_angles), + n_angles if negative, - n_angles if that gave n_angles
 *   v = rho / (float)resolution - 0.5f; a pixel with v > n_cells - 0.5 is 0; otherwise v = max(v, 0) (the half bin in front
 *       of the first bin centre reads bin 0)
 *   nearest:  a = rintf(u) (n_angles wraps to 0), b = min(rintf(v), n_cells - 1); the value is z(b, a)
 *   bilinear: a0 = floorf(u), fu = u - a0, a1 = a0 + 1 wrapped; b0 = floorf(v), fv = v - b0, b1 = min(b0 + 1, n_cells - 1);
 *             p0 = (1 - fu) * z(b0, a0) + fu * z(b0, a1), p1 likewise on b1, value = rintf((1 - fv) * p0 + fv * p1)
 * where z(b, a) reads azimuth a through the column mapping above; the value is saturated to u8.  theta_inc must be nonzero.
 * d_cart_u8 = [n][width][width]. */
int rr_polar_to_cartesian_device(rr_ctx* ctx, const uint8_t* d_imgs_u8, int n_frames, const rr_cartesian_config* cfg,
                                 uint8_t* d_cart_u8 /*[n][width][width]*/, void* stream);
int rr_polar_to_cartesian(rr_ctx* ctx, const uint8_t* imgs_u8, int n_frames, const rr_cartesian_config* cfg,
                          uint8_t* cart_u8);                                         /* host buffers, synchronous */

/* ---- object annotations: per-object extents and counts from label images (rr_notes.hip) ---------------------------
 * What every consumer of the label images does next: one record per object -- is it visible in this scan and with how many pixels,
 * where does it sit in range and azimuth, where is its strongest return, how much of what names it is a ghost or a multipath echo.
 * The reference has no such output: parity is UNPINNED and everything below is the build's own definition (a numpy restatement in
 * tests/notes_ref.py checks the kernels: every integer field bit for bit, the four floats to the ulps of cosf / sinf).
 * Inputs, in image layout with scroll applied (what the provenance call writes):
 *   labels uint32 [n][n_cells][n_angles]   info words (object id | pass << 24 | kind << 28) or RR_LABEL_NONE
 *   imgs   u8, same shape, or NULL         NULL reads as an image of zeros: peak and sum_intensity are 0
 *   n_objects                              records per frame; an id >= n_objects has no record
 *   extent_mask                            a mask of RR_NOTE_DIRECT | RR_NOTE_GHOST | RR_NOTE_MULTIPATH (0: the counts alone)
 * Class of a labelled pixel: RR_NOTE_MULTIPATH if kind is 1; otherwise RR_NOTE_GHOST if pass > 0; otherwise RR_NOTE_DIRECT.
 * Column to azimuth: column col holds azimuth a = (col - scroll_image) mod n_angles (the mapping of the point clouds above).
 * Output: one rr_object_note per (frame, object id) at d_notes[f * n_objects + id], every byte of it written (reserved words 0):
 *   n_direct, n_ghost, n_multipath   pixels naming the object, by class (always all three, whatever the mask)
 *   n_extent                         pixels whose class is in extent_mask; only these feed the fields below
 *   bin_min, bin_max                 range extent of those pixels; 0xFFFFFFFF and 0 when n_extent == 0
 *   az_begin, az_count               the smallest arc of AZIMUTHS (not columns) covering them, by the arc rule
 *   peak, peak_bin, peak_az          the largest image value among them and the bin and azimuth where it lies; equal values go to the lower
 *                                    bin, then the lower azimuth; all 0 when n_extent == 0
 *   sum_intensity                    sum of the image values over them
 *   x_min, x_max, y_min, y_max       min / max over them of r * cosf(theta) and r * sinf(theta), one f32 multiply each, with
 *                                    r = (float)(((double)bin + 0.5) * resolution) and theta = theta_min + (float)a * theta_inc exactly as
 *                                    a detected point's; +inf / -inf when n_extent == 0
 * Arc rule.  O = the set of azimuths that hold a pixel of the extent.  Take the longest circular run of azimuths outside O; among equal
 * longest runs the one whose first azimuth (walking upwards, so a run through azimuth 0 begins at its high end) is lowest.  az_begin is
 * the azimuth after that run, az_count = n_angles - the run's length: the arc is az_begin, az_begin + 1, .. (mod n_angles).  Every azimuth
 * occupied gives (0, n_angles), none (0, 0).
 * Skipped pixels.  A labelled pixel whose object id is >= n_objects feeds no record and is counted in d_skipped[f]; RR_LABEL_NONE is
 * not counted there.  Nothing is lost silently.
 * Every reduction is over integers or a min / max (the floats through an order-preserving integer mapping): a record does not depend on
 * the order of execution, two calls on the same planes return the same bytes.
 * Scratch is the caller's: rr_annotate_scratch_bytes bytes (64 per frame and object plus one bit per azimuth, frame and object), 16-byte
 * aligned like d_notes; its contents before the call do not matter and mean nothing afterwards.  Like the point clouds the device forms
 * write nothing but the caller's buffers, use no context-owned memory and read geometry and config BY VALUE when the call is made: they
 * may run on any stream beside batches in flight.  The host forms stage through context-owned buffers and are synchronous.
 * Out of scope: rr_multi has no annotation call (use the context of one device); parameter batches (the provenance chain is for pose
 * batches); velocities per object; oriented boxes.
 * Refused with a message and nothing written: -1 for a null ctx; -2 without a config (the simulate form also without a mesh, materials
 * or beam); -3 for a null required buffer, n_frames outside 1..65535 (the simulate form: 1..RR_MAX_BATCH), n_objects < 1 or >= 2^24 - 1,
 * unknown mask bits, n_cells > RR_LABEL_MAX_CELLS, n_angles > 65535, a scratch or record buffer that is not
 * 16-byte aligned, scratch_bytes below rr_annotate_scratch_bytes; the label-point call also for max_points < 0 and for a source plane
 * without its destination (or the reverse); the Cartesian call for what rr_polar_to_cartesian_device refuses and for interpolation != 0. */
#define RR_NOTE_DIRECT    1u
#define RR_NOTE_GHOST     2u
#define RR_NOTE_MULTIPATH 4u
typedef struct rr_object_note {       /* 80 B, five 16-B stores */
    uint32_t n_direct, n_ghost, n_multipath, n_extent;
    uint32_t bin_min, bin_max, az_begin, az_count;
    uint32_t peak, peak_bin, peak_az, reserved0_;
    uint64_t sum_intensity;
    float    x_min, x_max;
    float    y_min, y_max;
    uint32_t reserved1_[2];
} rr_object_note;
/* bytes of d_scratch for a call of that shape; 0 for a shape the calls refuse (a count below 1) */
size_t rr_annotate_scratch_bytes(int n_frames, int n_objects, int n_angles);
int rr_annotate_labels_device(rr_ctx* ctx, const uint32_t* d_labels /*[n][n_cells][n_angles]*/, const uint8_t* d_imgs_u8_or_NULL, int n_frames,
                              int n_objects, uint32_t extent_mask, rr_object_note* d_notes /*[n][n_objects]*/, uint32_t* d_skipped /*[n]*/,
                              void* d_scratch, size_t scratch_bytes, void* stream);
int rr_annotate_labels(rr_ctx* ctx, const uint32_t* labels, const uint8_t* imgs_u8_or_NULL, int n_frames, int n_objects, uint32_t extent_mask,
                       rr_object_note* out_notes, uint32_t* out_skipped);                 /* host buffers, synchronous */
/* The identity of detected points: for the first min(total, max_points) points of each frame (total = d_offsets[f][n_angles], the points
 * rr_detect_device wrote at d_points + f * max_points) the label, face and range rate at the point's (bin, column), at the point's index in
 * d_point_labels / d_point_faces / d_point_vel [n][max_points]; nothing is written past those points.  d_faces and d_vel_img (the velocity
 * image of the Doppler call) may be NULL, each together with its destination.  A point whose bin or column lies outside the image names
 * nothing: RR_LABEL_NONE, NaN.  One gather kernel, asynchronous on `stream`. */
int rr_label_points_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_offsets /*[n][n_angles+1]*/, int n_frames, int max_points,
                           const uint32_t* d_labels, const uint32_t* d_faces_or_NULL, const float* d_vel_img_or_NULL, uint32_t* d_point_labels,
                           uint32_t* d_point_faces, float* d_point_vel, void* stream);
/* The instance mask of a bird's-eye image: uint32 planes (labels, faces) resampled by the NEAREST rule of rr_polar_to_cartesian_device,
 * expression for expression, so pixel (i, j) of the mask names what pixel (i, j) of the nearest image shows; a pixel beyond the last bin
 * is RR_LABEL_NONE.  cfg->interpolation must be 0: ids do not interpolate.  d_cart_u32 = [n][width][width]. */
int rr_polar_to_cartesian_labels_device(rr_ctx* ctx, const uint32_t* d_planes_u32 /*[n][n_cells][n_angles]*/, int n_frames,
                                        const rr_cartesian_config* cfg, uint32_t* d_cart_u32, void* stream);
int rr_polar_to_cartesian_labels(rr_ctx* ctx, const uint32_t* planes_u32, int n_frames, const rr_cartesian_config* cfg,
                                 uint32_t* cart_u32);                                  /* host buffers, synchronous */
/* Ground-truth generation in one call: a provenance chain for n_frames (1..RR_MAX_BATCH) poses, then the annotation of its label planes with
 * its images, on the context's stream; n_objects is the mesh's (the largest face_object_id + 1).  Only the records and skip counts (and
 * the images, if out_imgs_u8 is not NULL: the bytes of rr_simulate_batch_device) reach the host; no label plane leaves the GPU.
 * out_notes [n][n_objects], out_skipped [n] (always 0 here: every id is the mesh's).  Synchronous; the frame errors -7 / -8 are returned
 * before anything is written. */
int rr_simulate_batch_annotations(rr_ctx* ctx, const float* poses, int n_frames, uint32_t extent_mask, uint8_t* out_imgs_u8_or_NULL,
                                  rr_object_note* out_notes, uint32_t* out_skipped);

/* ---- translation registration (rr_shift.hip) ----------------------------------------------------------------------
 * rr_align_images settles the yaw; the other two degrees of freedom of a planar pose, x and y, are to first order a
 * translation of the Cartesian bird's-eye image (rr_polar_to_cartesian).  One exact 2-D cross-correlation over a window of
 * pixel shifts replaces a grid of simulated positions.  The reference has no registration step: this is the build's own
 * definition, unpinned by anything the reference holds.
 * Images are uint8 [H][W], row-major; n images x_k are compared with one reference r.  H = height, W = width and
 * S = max_shift are call arguments: the call depends on no config and no mesh.  T is the template window, rows [S, H-S) by
 * columns [S, W-S), N = (H-2S)(W-2S) pixels; every index of r below is in range, nothing wraps and nothing is padded.
 * For dy, dx in -S..S:
 *   xcorr[dy][dx] = sum over (i,j) in T of x[i][j] * r[i+dy][j+dx]                           exact int64
 *   (dy, dx) is where the content of x is found in r.
 * Sx, Sxx are the sums of x and x^2 over T; Sr[dy][dx], Srr[dy][dx] the sums of r and r^2 over T moved by (dy, dx) (box sums
 * of the reference, computed once per call and shared by all n images).  All exact uint64.
 *   sse[d]  = Sxx + Srr[d] - 2 xcorr[d]                                                      exact uint64
 *   psnr    = from sse and N with the expression of rr_score_images_device (+inf at sse == 0)
 *   ncc[d]  = (N xcorr[d] - Sx Sr[d]) / sqrt((N Sxx - Sx^2)(N Srr[d] - Sr[d]^2)): the numerator and the two factors are exact
 *             int64, converted to f64, then one multiply, one sqrt, one divide; 0 when either factor is 0
 *   best    = the shift with the smallest sse (NOT the largest xcorr: Srr depends on the shift); a tie goes to the smallest
 *             index (dy+S)(2S+1) + (dx+S); n_best = the number of shifts that attain it
 *   sub_dy, sub_dx = 0.5 (e[-1] - e[+1]) / (e[-1] - 2 e[0] + e[+1]) along each axis at the best shift, e = sse: numerator and
 *             denominator are exact integers, converted to f64, the numerator halved, one divide; 0 when a neighbour lies
 *             outside -S..S or the denominator is <= 0
 * A record holds xcorr, sse, psnr, ncc, sum_r and sum_rr AT the best shift, and the SSE of its four neighbours (UINT64_MAX
 * where a neighbour lies outside -S..S).  d_xcorr and d_sse (HBM, [n_images][2S+1][2S+1], index [dy+S][dx+S], or NULL)
 * receive the whole surfaces.  Synchronous on `stream`, context-owned scratch, one set per stream the call has been made on,
 * more than 64 images in chunks: the conventions of rr_align_images_device.
 * Limits: H, W in 1..8192; 0 <= S <= 64; H > 2S and W > 2S; N <= 2^23 (which keeps N xcorr inside int64); n_images 1..65535.
 * Refused with a message and nothing written: -3 for a null buffer or an argument outside these limits.
 * Pose meaning.  rr_polar_to_cartesian puts pixel (i, j) at forward (c - i) pixel_size and left (c - j) pixel_size, and a
 * world point p seen from pose t lies at p - t in the sensor frame.  So if x was rendered at t_x and r taken at t_r with the
 * same yaw, content moves by t_x - t_r, which in metres is (-dy, -dx) pixel_size.  The correction to ADD to the simulated
 * pose, in the sensor's own (forward, left) axes, is therefore (+dy pixel_size, +dx pixel_size). */
typedef struct rr_shift_record {   /* 128 B */
    int32_t dy, dx, n_best, reserved_;
    int64_t xcorr;            /* at (dy, dx) */
    uint64_t sse;             /* at (dy, dx) */
    double psnr, ncc;         /* at (dy, dx) */
    double sub_dy, sub_dx;    /* sub-pixel offsets to add to dy, dx */
    uint64_t sse_nb[4];       /* sse at dy-1, dy+1, dx-1, dx+1; UINT64_MAX outside -S..S */
    uint64_t sum_x, sum_xx;   /* over T */
    uint64_t sum_r, sum_rr;   /* over T moved by (dy, dx) */
} rr_shift_record;
int rr_shift_images_device(rr_ctx* ctx, const uint8_t* d_imgs_u8, int n_images, const uint8_t* d_ref_u8, int height, int width,
                           int max_shift, rr_shift_record* out /* host [n_images] */,
                           int64_t* d_xcorr /* HBM [n_images][2S+1][2S+1], or NULL */,
                           uint64_t* d_sse /* HBM [n_images][2S+1][2S+1], or NULL */, void* stream);
/* The host-buffer form: imgs_u8 [n_images][H][W], ref_u8 [H][W], xcorr and sse host [n_images][2S+1][2S+1] or NULL.
 * Synchronous; staged 64 images at a time, the records written once all of them are done, the surfaces chunk by chunk. */
int rr_shift_images(rr_ctx* ctx, const uint8_t* imgs_u8, int n_images, const uint8_t* ref_u8, int height, int width, int max_shift,
                    rr_shift_record* out, int64_t* xcorr, uint64_t* sse);
/* rr_simulate_batch_device into a context-owned image buffer, rr_polar_to_cartesian_device on the n images and on
 * ref_polar_u8 (host, [n_cells][n_angles]), then rr_shift_images_device with H = W = cfg->width: one simulated pose in, its
 * translation against the real scan out.  n_frames is 1..RR_MAX_BATCH; out_cart_u8 (host, [n_frames][width][width]) or NULL,
 * and with NULL no image leaves the GPU; xcorr host [n_frames][2S+1][2S+1] or NULL.  Refusals: those of
 * rr_simulate_batch_align, rr_polar_to_cartesian and rr_shift_images_device. */
int rr_simulate_batch_shift(rr_ctx* ctx, const float* poses, int n_frames, const uint8_t* ref_polar_u8, const rr_cartesian_config* cfg,
                            int max_shift, uint8_t* out_cart_u8, rr_shift_record* out, int64_t* xcorr);

/* ---- place recognition: polar ring/sector descriptors and exact matching (rr_place.hip) ------------------------------
 * rr_align_images and rr_shift_images refine a pose that is already close.  "Where on this map was this scan taken" is
 * answered by a database: render the map once on a grid of poses, keep a compact signature of every rendered scan, look a
 * real scan up in it.  The reference has no such step: the definitions below are the build's own, unpinned by anything
 * the reference holds.
 * Descriptor.  rr_place_config {cell_begin, cell_end, n_rings = R, n_sectors = S}; L = cell_end - cell_begin, A = n_angles.
 *   ring r   = the cells [cell_begin + floor(r L / R), cell_begin + floor((r+1) L / R))
 *   sector j = the image columns [floor(j A / S), floor((j+1) A / S)), as they lie in the image: scroll_image is not undone,
 *              a shift of the match takes care of it
 *   d[r][j]  = floor(sum of the pixels of the rectangle / pixel count of the rectangle): the sum is an exact integer, the
 *              result a uint8
 * Layout uint8 [R][S]: a descriptor is itself a tiny polar image of K = R S bytes.
 * Limits: 1 <= R <= 64, 4 <= S <= 128, S <= A, R <= L, R S <= 8192, 0 <= cell_begin < cell_end <= n_cells.
 * Match.  The definition of rr_align_images on descriptors, n_query queries against n_db candidates.  For query q and
 * candidate c, both [R][S]:
 *   xcorr[s] = sum_r sum_j q[r][j] c[r][(j+s) mod S] = sum(np.roll(q, s, axis=1) * c)              exact
 *              s is the number of sectors to ADD to the query's scroll so that it lines up with the candidate, the direction
 *              of rr_align_images
 *   sse[s]   = Sqq + Scc - 2 xcorr[s]                                    exact, fits 32 bits: 2 * 255^2 * 8192 < 2^31
 *   best     = the smallest s with the largest xcorr; n_best = the number of shifts that attain it
 *   ncc      = (K xcorr - Sq Sc) / sqrt((K Sqq - Sq^2)(K Scc - Sc^2)) at the best shift: numerator and factors exact int64,
 *              converted to f64, then one multiply, one sqrt, one divide; 0 when either factor is 0
 *   psnr     = from sse over K pixels with the expression of rr_score_images_device (+inf at sse == 0)
 * Ranking.  Candidates are ranked by the exact 64-bit key (sse at the best shift) << 32 | candidate index, ascending: equal
 * SSE goes to the lower index, duplicates in the database are legal.  The call returns the top_k smallest,
 * 1 <= top_k <= min(32, n_db), as records [n_query][top_k] on the host.  Ranking uses integers only.  Ranking by NCC is
 * deliberately not offered: a caller for whom gain differences between real and simulated images matter re-ranks the top_k
 * by the returned ncc.
 * d_sse (HBM, uint32 [n_query][n_db], or NULL) receives every pair's SSE at its best shift, d_shift (HBM, uint16
 * [n_query][n_db], or NULL; only together with d_sse) that shift.
 * Limits: 1 <= n_query <= 64, 1 <= n_db <= 2^28.  Synchronous on `stream`, context-owned scratch, one set per stream the call has
 * been made on: the conventions of rr_align_images_device.  The database may start at any byte.
 * Refused with a message and nothing written: -2 without a config where one is needed (the describe calls), -3 for a null
 * buffer, an argument outside these limits, top_k > n_db, d_shift without d_sse.
 * Pose meaning.  The shift moves the QUERY's sectors: by the rule of rr_align_images the query's pose turned by
 * -s (A / S) theta_inc about the sensor's z axis is the candidate's, and the candidate's pose turned by +s (A / S) theta_inc
 * is the query's (s wrapped into (-S/2, S/2]).  Exact only when S divides A: otherwise sector widths differ by one column. */
typedef struct rr_place_config {
    int32_t cell_begin, cell_end;   /* the window of cells the rings divide */
    int32_t n_rings, n_sectors;     /* R, S */
} rr_place_config;
typedef struct rr_place_match {   /* 40 B, no padding */
    uint32_t index;           /* the candidate */
    int32_t shift;            /* sectors to add to the query's scroll */
    uint32_t sse;             /* at `shift` */
    uint32_t n_best;          /* shifts that attain the largest xcorr */
    int64_t xcorr;            /* at `shift` */
    double ncc, psnr;         /* at `shift` */
} rr_place_match;
/* n images [n][n_cells][n_angles] in HBM -> descriptors [n][R][S] in HBM; enqueued on `stream`, not synchronised.  Needs a
 * config (the image shape) and no mesh.  n is 1..65535. */
int rr_describe_images_device(rr_ctx* ctx, const uint8_t* d_imgs_u8, int n, const rr_place_config* cfg, uint8_t* d_desc, void* stream);
/* The host-buffer form, staged 64 images at a time; synchronous. */
int rr_describe_images(rr_ctx* ctx, const uint8_t* imgs_u8, int n, const rr_place_config* cfg, uint8_t* desc);
/* rr_simulate_batch_device into a context-owned image buffer, then rr_describe_images_device: n_frames (1..RR_MAX_BATCH)
 * poses in, out_desc (host, [n_frames][R][S]) out.  R S bytes per pose leave the GPU instead of an image. */
int rr_simulate_batch_describe(rr_ctx* ctx, const float* poses, int n_frames, const rr_place_config* cfg, uint8_t* out_desc);
/* d_query [n_query][R][S] and d_db [n_db][R][S] in HBM -> out (host, [n_query][top_k]).  Needs neither a config nor a mesh. */
int rr_match_descriptors_device(rr_ctx* ctx, const uint8_t* d_query, int n_query, const uint8_t* d_db, int n_db, int n_rings, int n_sectors,
                                int top_k, rr_place_match* out /* host [n_query][top_k] */, uint32_t* d_sse /* HBM [n_query][n_db], or NULL */,
                                uint16_t* d_shift /* HBM [n_query][n_db], or NULL */, void* stream);
/* The host-buffer form: the database is staged in chunks and a running top_k kept; sse and shift host [n_query][n_db] or NULL. */
int rr_match_descriptors(rr_ctx* ctx, const uint8_t* query, int n_query, const uint8_t* db, int n_db, int n_rings, int n_sectors, int top_k,
                         rr_place_match* out, uint32_t* sse, uint16_t* shift);

/* ---- sweep compensation: motion and Doppler distortion taken out again (rr_deskew.hip) -------------------------------
 * rr_set_motion_poses gives every azimuth its own sensor pose and the Doppler call draws an echo gain * v_r metres from where the mesh
 * puts it: the two distortions of a moving spinning FMCW radar (MulRan, Boreas, Oxford).  The calls below are their inverse: points and
 * bird's-eye images in ONE rigid frame, the reference pose's.  The reference has no such step: parity is UNPINNED and everything below is
 * the build's own definition (a numpy restatement in tests/deskew_ref.py checks the kernels).  All f32, nothing fused, the quaternion
 * algebra in the term order of rmagine's (rr_device.h: q_mul, q_conj, q_rot, v_sub, v_add, v_scale, v_dot).  Geometry (n_angles, theta_min,
 * theta_inc, resolution, n_cells) and scroll_image are read BY VALUE when a call is made, as in rr_detect*.
 * The record of frame f and azimuth a, from az_poses[f][a] = (q_a, t_a) (map from sensor: the table rr_set_motion_poses takes), the
 * reference pose ref_poses[f] = (q_ref, t_ref), and optionally the sensor's map-frame velocity v_s = sensor_vel[f] and `gain`, both with
 * the meaning they have in the Doppler call:
 *     q = q_mul(q_conj(q_ref), q_a)                 t = q_rot(q_conj(q_ref), v_sub(t_a, t_ref))
 *     theta = theta_min + (float)a * theta_inc      u = q_rot(q_a, (cosf(theta), sinf(theta), 0))
 *     v_r = -(v_dot(v_s, u))                        (the Doppler section's dL/dt for a direct echo off a static object)
 *     dr = gain * v_r                               sensor_vel == NULL or gain == 0: dr = 0 exactly
 * The device form cannot look at device data: it checks nothing about the poses, the velocities or the table's contents (a non-finite
 * record gives NaN points and 0 pixels, never an access outside the buffers); the host form refuses them.  d_table and every other
 * rr_sweep_rec device buffer must be 16-byte aligned.
 * Compensated points.  For each of the min(d_offsets[f][n_angles], max_points) points of frame f (what rr_detect_device wrote):
 *     a = (column - scroll_image) mod n_angles, rec = table[f][a]
 *     r = (float)(((double)bin + 0.5) * resolution)  (the detector's own range)      rc = r - rec.dr
 *     p = v_scale((x, y, z), rc / r)                 out.xyz = v_add(q_rot(rec.q, p), rec.t)
 *   intensity, column and bin are copied; one output per input in the same order, so d_offsets stays valid for the output; d_out may
 *   equal d_points.  A point with rc <= 0 or non-finite, or whose column lies outside the image, gets x = y = z = NaN.  Slots beyond the
 *   count are not touched.  The kernel reads the counts on the device: no host round trip.
 * Compensated Cartesian image: the bird's-eye image in the REFERENCE frame.  Pixel (i, j) sits at P = (x, y, 0) exactly as in
 * rr_polar_to_cartesian; "u from phi" below is that call's formula for u, "wrapped" its n_angles -> 0.
 *     a_0 = rintf(u), wrapped, with u from phi = atan2f(y, x)                 (the uncompensated nearest rule)
 *     for k = 1 .. iterations:  rec = table[f][a_{k-1}];  Q = q_rot(q_conj(rec.q), v_sub(P, rec.t));  phi = atan2f(Q.y, Q.x);
 *                               u from phi;  a_k = rintf(u), wrapped
 *     with the rec, Q and u of the last step:  rho = sqrtf(v_dot(Q, Q))  (the slant range: the fan is wide in elevation)
 *                               rho_m = rho + rec.dr  (a gather runs the forward model);  v = rho_m / (float)resolution - 0.5f
 *     the value is sampled at (u, v) exactly as rr_polar_to_cartesian does (v > n_cells - 0.5 gives 0, v clamped at 0, the column
 *     mapping, nearest / bilinear, rintf, saturation); a non-finite or negative rho_m gives 0.
 *   The iteration count is fixed, so the result is a definition, not a tolerance.  At the sweep seam (between the last and the first
 *   azimuth) a pixel of the reference frame may have been seen twice or not at all; the iteration returns what it returns there.  With an
 *   identity table (q = (0, 0, 0, 1), t = 0, dr = 0) the result equals rr_polar_to_cartesian_device byte for byte for every `iterations`.
 * Like the point clouds the device forms write nothing but the caller's buffers, use no context-owned memory and may run on any stream
 * beside batches in flight.  The host forms stage through context-owned buffers and are synchronous.
 * Refused with a message and nothing written: -1 for a null ctx; -2 without a config; -3 for a null required buffer, n_frames outside
 * 1..65535, a table that is not 16-byte aligned, max_points < 0, iterations outside 1..8, n_angles * 32 > 65536 (the Cartesian call keeps a
 * frame's records in LDS), what rr_polar_to_cartesian_device refuses, a non-finite gain; rr_sweep_table (host form) also for a non-finite
 * pose or velocity and for a quaternion whose squared norm is off 1 by more than 1e-3. */
typedef struct rr_sweep_rec {   /* 32 B, two 16-B stores */
    float q[4];   /* x,y,z,w: rotation from the sensor frame of this azimuth into the reference frame */
    float t[3];   /* translation of the same transform, metres */
    float dr;     /* metres to SUBTRACT from a measured range of this azimuth: gain * v_r of a static world */
} rr_sweep_rec;
int rr_sweep_table_device(rr_ctx* ctx, const float* d_az_poses /*[n][n_angles][7]*/, const float* d_ref_poses /*[n][7]*/,
                          const float* d_sensor_vel_or_NULL /*[n][3]*/, float gain, int n_frames, rr_sweep_rec* d_table /*[n][n_angles]*/,
                          void* stream);
int rr_sweep_table(rr_ctx* ctx, const float* az_poses, const float* ref_poses, const float* sensor_vel_or_NULL, float gain, int n_frames,
                   rr_sweep_rec* table);                                                 /* host buffers, synchronous */
int rr_compensate_points_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_offsets /*[n][n_angles+1]*/, int n_frames,
                                int max_points, const rr_sweep_rec* d_table, rr_radar_point* d_out /* may equal d_points */, void* stream);
int rr_compensate_points(rr_ctx* ctx, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points,
                         const rr_sweep_rec* table, rr_radar_point* out);                /* host buffers, synchronous */
int rr_polar_to_cartesian_sweep_device(rr_ctx* ctx, const uint8_t* d_imgs_u8, int n_frames, const rr_cartesian_config* cfg,
                                       const rr_sweep_rec* d_table, int iterations /*1..8*/, uint8_t* d_cart_u8 /*[n][width][width]*/,
                                       void* stream);
int rr_polar_to_cartesian_sweep(rr_ctx* ctx, const uint8_t* imgs_u8, int n_frames, const rr_cartesian_config* cfg, const rr_sweep_rec* table,
                                int iterations, uint8_t* cart_u8);                       /* host buffers, synchronous */

/* ---- scan matching: rigid 2-D registration of point clouds (rr_icp.hip) ------------------------------------------------
 * Batched point-to-point ICP in the plane with a FIXED iteration count: which SE(2) moves each of n source clouds onto ONE target cloud.
 * The reference has no such step: parity is UNPINNED and everything below is the build's own definition (a numpy restatement in
 * tests/icp_ref.py checks the kernels bit for bit).  All f32 arithmetic is un-fused.
 * Source frame f is what rr_detect_device or rr_compensate_points_device wrote at d_points + f * max_points; its count is
 * min(d_offsets[f][n_angles], max_points), read on the device with no host round trip.  The target is
 * d_tgt_points[0 .. min(*d_tgt_count, max_tgt)), d_tgt_count a device uint32_t* (a caller passes &offsets[g][n_angles] of any detected
 * frame).  z, intensity, column and bin are ignored.  The source may alias the target.
 * The state per frame is (c, s, tx, ty) in f64: the transform q ~ R p + t that maps a source point into the target's frame.
 * d_init [n][4] f64 holds the initial states; NULL means identity.  (c, s) of an initial state is normalised once by
 * hypot = sqrt(c*c + s*s); a non-finite or zero hypot is refused by the host form, and in the device form sets RR_ICP_DEGENERATE and
 * makes the state the identity.
 * One CORRESPONDENCE PASS for a state:
 *   1. cf, sf, txf, tyf are the state rounded to f32.  For source point i:
 *          px = (cf*x - sf*y) + txf            py = (sf*x + cf*y) + tyf
 *   2. best = +inf, j* = NONE.  For j ascending over the target: dx = px - Tx[j], dy = py - Ty[j], d2 = dx*dx + dy*dy; take j iff
 *      d2 < best.  So ties go to the lower index and a NaN never wins.  A target point with a non-finite coordinate, or with
 *      |coordinate| >= 8192, is never a candidate.
 *   3. Point i is MATCHED iff px and py are finite and below 8192 in magnitude, j* != NONE, and best <= gate2, gate2 = gate * gate in f32.
 *   4. The matched pairs are quantised: P = (int32)rintf(p * 256.0f) per coordinate of (px, py); Q likewise from the target's coordinates.
 *   5. These int64 sums run over the matched pairs: N, SPx, SPy, SQx, SQy, Sdot = sum(Px*Qx + Py*Qy), Scross = sum(Px*Qy - Py*Qx),
 *      Ssse = sum((Px-Qx)^2 + (Py-Qy)^2).  With at most 65,536 points and |P| <= 2^21 no sum overflows; integer sums make the result
 *      independent of order.
 * One SOLVE is f64 arithmetic only (+ - * / sqrt, no trigonometry).  Every sum is converted to f64 first, the expressions are
 * evaluated as written:
 *     A = N*Sdot - (SPx*SQx + SPy*SQy)         B = N*Scross - (SPx*SQy - SPy*SQx)         h = sqrt(A*A + B*B)
 *     if N < 2 or !(h > 0):  flags |= RR_ICP_DEGENERATE  (the state keeps its value in this iteration)
 *     else:  dc = A/h   ds = B/h   mpx = (SPx/N)/256  (likewise mpy, mqx, mqy)
 *            dtx = mqx - (dc*mpx - ds*mpy)     dty = mqy - (ds*mpx + dc*mpy)
 *            c' = dc*c - ds*s    s' = ds*c + dc*s    tx' = (dc*tx - ds*ty) + dtx    ty' = (ds*tx + dc*ty) + dty
 *            (c', s') divided by sqrt(c'*c' + s'*s')
 * The call runs `iterations` times (pass, solve), then one last pass at the final state.  The count is fixed: a definition, not a
 * tolerance.  iterations = 0 scores the initial states only (a point-cloud likelihood for n hypotheses); no solve runs then, so
 * RR_ICP_DEGENERATE can only come from an initial state.
 * Output per frame is one rr_icp_rec from the last pass: the state, sse = Ssse, n_matched = N, flags (RR_ICP_DEGENERATE is sticky;
 * RR_ICP_TRUNCATED: the source's or the target's count exceeded its max).  Optionally d_corr [n][max_points] uint32 receives the last
 * pass's j* per source point, 0xFFFFFFFF for an unmatched point (also one whose nearest lies beyond the gate); nothing is written past
 * a frame's count.  NULL: not wanted.
 * The device form enqueues 2 * iterations + 3 launches on `stream` (the initial states, the pairs, the last pass and the step that
 * writes the record) with no host round trip between them.  It touches no context memory but a scratch accumulator of 64 bytes per frame
 * that the context keeps PER STREAM (it grows with the largest n_frames seen on that stream; growing it drains that stream), so it
 * may run on any stream beside batches in flight, and calls on different streams may overlap.  d_init and d_recs must be 8-byte aligned.
 * The host form stages through context-owned buffers and is synchronous; its tgt_count is a value.
 * Refused with a message and nothing written: -1 for a null ctx; -2 without a config (n_angles is the offsets' stride); -3 for a null
 * required buffer, n_frames outside 1..65535, max_points or max_tgt outside 0..65536, iterations outside 0..64, a gate that is not
 * finite and positive, a misaligned d_init or d_recs; the host form also for an initial state whose hypot is zero or not finite. */
#define RR_ICP_DEGENERATE 1u   /* a solve had fewer than 2 matched pairs or no direction (h == 0), or the initial state had no direction */
#define RR_ICP_TRUNCATED 2u    /* the source's or the target's count exceeded max_points / max_tgt: the cloud was cut */
typedef struct rr_icp_rec {    /* 48 B */
    double c, s, tx, ty;       /* q ~ [c -s; s c] p + (tx, ty): source frame into target frame; c*c + s*s = 1 up to rounding */
    int64_t sse;               /* Ssse of the last pass, in (1/256 m)^2 */
    uint32_t n_matched;        /* N of the last pass */
    uint32_t flags;            /* RR_ICP_* */
} rr_icp_rec;
int rr_register_points_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_offsets /*[n][n_angles+1]*/, int n_frames,
                              int max_points, const rr_radar_point* d_tgt_points, const uint32_t* d_tgt_count, int max_tgt,
                              const double* d_init_or_NULL /*[n][4]*/, float gate, int iterations /*0..64*/, rr_icp_rec* d_recs /*[n]*/,
                              uint32_t* d_corr_or_NULL /*[n][max_points]*/, void* stream);
int rr_register_points(rr_ctx* ctx, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points,
                       const rr_radar_point* tgt_points, uint32_t tgt_count, int max_tgt, const double* init_or_NULL, float gate, int iterations,
                       rr_icp_rec* recs, uint32_t* corr_or_NULL);                        /* host buffers, synchronous */
/* the blocking of k_icp_pass: source points per workgroup and (x, y) pairs per LDS tile of the target (tests put counts at their edges) */
void rr_icp_tile_sizes(int* source_tile, int* target_tile);

/* ---- likelihood field: exact distance map and pose-batch scoring (rr_field.hip) ------------------------------------------
 * The sensor model of a particle filter, and of a dense search over a lattice of (x, y, yaw): very many pose hypotheses for ONE observed
 * scan scored against a map.  The map's points are rasterised once, the exact Euclidean distance transform is taken once, and a hypothesis
 * then costs one table look-up per point.  The reference has no such step: parity is UNPINNED and everything below is the build's own
 * definition (a numpy restatement in tests/field_ref.py checks the kernels bit for bit).  All f32 arithmetic is un-fused; every result is
 * an integer and independent of order.
 * POSE CONVENTION, stated once: a state (c, s, tx, ty) maps a cloud's sensor frame into the MAP frame, q = [c -s; s c] p + (tx, ty).  The
 * rasteriser's states place keyframe clouds in the map; a hypothesis state of rr_score_poses places the observed scan in the map.
 * GRID.  rr_field_config gives the shape.  The cell of a point (x, y) in the map frame:
 *     u = (x - x0) / cell      v = (y - y0) / cell                                    in f32
 *     the point is IN GRID iff u and v are finite, u >= 0 && u < (float)width and v >= 0 && v < (float)height; the comparisons are made
 *     in float, before any conversion to int
 *     ix = (int)floorf(u)      iy = (int)floorf(v)      linear index = iy * width + ix
 * 1. rr_rasterize_points[_device]: clouds into an occupancy grid.  The clouds are laid out as rr_detect_device /
 *    rr_compensate_points_device write them; the count of frame f is min(d_offsets[f][n_angles], max_points), read on the device; z,
 *    intensity, column and bin are ignored.  d_states has the layout and meaning of rr_register_points_device's d_init: (c, s, tx, ty) f64
 *    per frame, source frame into map frame; NULL means the identity.  States are used as given, rounded to f32 (cf, sf, txf, tyf); there
 *    is no normalisation here (a record of rr_register_points is already normalised: its first 32 bytes are a state).  The mapping is
 *    step 1 of the scan matcher:
 *        px = (cf*x - sf*y) + txf            py = (sf*x + cf*y) + tyf
 *    Every point that is IN GRID writes 1 into its cell; a point whose transformed coordinate is not finite is skipped.  The call only
 *    ever writes ones, into a buffer that the caller zeroed: several calls accumulate a map from keyframes, whatever their order.
 * 2. rr_distance_field[_device]: the exact saturated squared distance transform.  A cell is occupied iff occ >= threshold (so a thresholded
 *    Cartesian image from rr_polar_to_cartesian is a valid map as well).  With cap2 = max_dist * max_dist:
 *        field[iy][ix] = min(cap2, min over occupied cells (jx, jy) of (ix-jx)^2 + (iy-jy)^2)
 *    The minimum is an exact integer; an empty map is cap2 everywhere.  d_field_u16 must not alias d_occ_u8.
 * 3. rr_score_poses[_device]: the hot path.  The scan is ONE cloud, d_points[0 .. min(*d_count, max_points)), its count read on the device
 *    (a caller passes &offsets[g][n_angles] of a detected frame); it is shared by all hypotheses.  d_states [n_hyp][4] is f32 (c, s, tx, ty),
 *    used as given: no normalisation and no trigonometry on the device.  For hypothesis h and point i: the mapping above in f32, the
 *    cell rule, the look-up, and three integer sums into one rr_field_rec:
 *        sum_d2 over ALL points of the scan: the field value of an IN GRID point, cap2 for any other point
 *        n_in   the points IN GRID                    n_hit  the points IN GRID whose field value <= gate * gate
 *    A state that holds a NaN makes every point "not IN GRID": the hypothesis costs count * cap2 and no flag is needed.  With at most
 *    65,536 points sum_d2 < 2^33.  A count of 0 gives all-zero records.  Lower sum_d2 is better; turning it into a likelihood, e.g.
 *    exp(-sum_d2 * cell^2 / (2 sigma^2)), is the caller's job on the host.
 * The device forms enqueue on `stream` (NULL: the context's) with no host round trip, and use NO context-owned memory at all: they may run on
 * any stream beside batches in flight, and calls on different streams may overlap.  rr_rasterize_points_device is one launch,
 * rr_distance_field_device two (columns, rows), rr_score_poses_device one.  The host forms stage through context-owned buffers and are
 * synchronous; rr_rasterize_points reads occ_u8 as well as writing it (it accumulates), and rr_score_poses takes the scan's count as a value.
 * Refused with a message and nothing written: -1 for a null ctx; -2 for the rasteriser without a config (n_angles is the offsets' stride);
 * -3 for a null required buffer, a config field outside its stated range or a non-finite cell, x0 or y0, n_frames outside 1..65535,
 * max_points outside 0..65536, n_hyp outside 1..2^22, threshold outside 1..255, d_states misaligned for its element type (8 bytes for the
 * rasteriser's f64, 4 for the scorer's f32) or d_recs not 8-byte aligned. */
typedef struct rr_field_config {   /* 32 B */
    int32_t width, height;   /* cells, 1..4096 each */
    float   cell;            /* metres per cell, finite, > 0 */
    float   x0, y0;          /* map-frame coordinate of the low corner of cell (ix = 0, iy = 0), finite */
    int32_t max_dist;        /* saturation in cells, 1..255; cap2 = max_dist * max_dist <= 65025 */
    int32_t gate;            /* 0..max_dist: a point is a HIT iff its field value <= gate * gate */
    int32_t reserved_;
} rr_field_config;
typedef struct rr_field_rec {  /* 16 B */
    uint64_t sum_d2;   /* over ALL points of the scan: the field value of an IN GRID point, cap2 for any other point */
    uint32_t n_in;     /* points IN GRID */
    uint32_t n_hit;    /* points IN GRID whose field value <= gate * gate */
} rr_field_rec;
int rr_rasterize_points_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_offsets /*[n][n_angles+1]*/, int n_frames,
                               int max_points, const double* d_states_or_NULL /*[n][4]*/, const rr_field_config* cfg,
                               uint8_t* d_occ_u8 /*[height][width]*/, void* stream);
int rr_rasterize_points(rr_ctx* ctx, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points,
                        const double* states_or_NULL, const rr_field_config* cfg, uint8_t* occ_u8);     /* host buffers, synchronous */
int rr_distance_field_device(rr_ctx* ctx, const uint8_t* d_occ_u8, int threshold /*1..255*/, const rr_field_config* cfg,
                             uint16_t* d_field_u16 /*[height][width]*/, void* stream);
int rr_distance_field(rr_ctx* ctx, const uint8_t* occ_u8, int threshold, const rr_field_config* cfg, uint16_t* field_u16);   /* host buffers */
int rr_score_poses_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_count, int max_points,
                          const float* d_states /*[n_hyp][4]: c, s, tx, ty*/, int n_hyp /*1..2^22*/, const uint16_t* d_field_u16,
                          const rr_field_config* cfg, rr_field_rec* d_recs /*[n_hyp]*/, void* stream);
int rr_score_poses(rr_ctx* ctx, const rr_radar_point* points, uint32_t count, int max_points, const float* states, int n_hyp,
                   const uint16_t* field_u16, const rr_field_config* cfg, rr_field_rec* recs);           /* host buffers, synchronous */
/* the blocking of the kernels: points a wave of k_field_score takes per step, hypotheses per workgroup of it, cells of a row per sweep of
 * the transform's row pass (tests put counts and sizes at their edges) */
void rr_field_tile_sizes(int* points_tile, int* hyps_per_group, int* row_tile);

/* ---- occupancy mapping: posed scans fused into a log-odds grid (rr_occupancy.hip) -----------------------------------------
 * The map under the likelihood field, made from evidence rather than from single detections: rr_rasterize_points writes a 1 into every
 * cell any detection ever fell into, so one false alarm is a wall for ever, free space is not known at all and a wall seen 64 times
 * weighs what a phantom seen once does.  Here a detection ADDS evidence to its cell, the free space a scan swept SUBTRACTS it, and the
 * sum is thresholded.  The reference has no such step: parity is UNPINNED and everything below is the build's own definition (a numpy
 * restatement in tests/occupancy_ref.py checks the kernels).  All f32 arithmetic is un-fused; every result is an integer and independent
 * of order.
 * GRID.  rr_field_config, its IN GRID rule and its cell index (above) are reused unchanged; max_dist and gate are IGNORED here (any
 * value passes), so an evidence grid's map can be turned into a field on the same config.  The centre of cell (ix, iy), in f32:
 *     qx = x0 + ((float)ix + 0.5f) * cell          qy = y0 + ((float)iy + 0.5f) * cell
 * STATES are the rasteriser's: (c, s, tx, ty) f64 per scan, sensor frame into the map frame, rounded to f32 (cf, sf, txf, tyf) and used
 * as given; NULL means the identity.
 * EVIDENCE is int32 [height][width], zeroed by the caller; calls accumulate into it.  It holds plain, unsaturated sums, so neither the
 * order of the scans nor the order of the calls matters.  Keeping a cell's sum within int32 is the caller's job: one call moves a cell
 * down by at most n_frames * l_free (at most 65,535 * 127 < 2^23) and up by l_hit for every point that falls into it, so evidence
 * cannot wrap while 127 * (all points ever fused + all scans ever fused) < 2^31, about 16.9 million points.
 * rr_occupancy_update[_device] takes n scans laid out as rr_detect_device / rr_compensate_points_device write them (counts and offsets
 * are read on the device; x, y and bin of a point are used) and runs three steps:
 * 1. PROFILE.  Per scan f and image column col, with azimuth a = col - scroll (mod n_angles): the points of a column are sorted by bin,
 *    so its FIRST detection is the point at index d_offsets[f][col], if the column has any (d_offsets[f][col + 1] > d_offsets[f][col]) and
 *    that index is below max_points; fb is that point's bin.  fb = n_cells for a column with no detection.  A column whose detections
 *    were all cut by max_points asserts nothing: its free_bins is 0.  Otherwise
 *        free_bins = min(max(fb - margin_bins, 0), max_free_bin)
 *        r = (float)((double)free_bins * resolution)          free2[f][a] = r * r              in f32
 *    The profile goes to the caller's buffer d_profile, float [n][n_angles]: the device form uses no context memory.
 * 2. FREE SPACE, the hot path.  Per cell and scan, all f32:
 *        dx = qx - txf      dy = qy - tyf      px = cf*dx + sf*dy      py = cf*dy - sf*dx
 *        u = the azimuth coordinate of atan2f(py, px) (that of rr_polar_to_cartesian: (phi - theta_min) / theta_inc mod n_angles)
 *        a = the nearest azimuth index, rintf(u) mod n_angles          rho2 = px*px + py*py
 *    The cell is FREE in that scan iff rho2 < free2[f][a]: ranges are compared squared.  A non-finite px or py is never free.
 *        evidence[cell] -= l_free * (the number of scans of the call in which the cell is free)
 *    atan2f is the device library's; the restatement's differs from it in the last place, which moves a cell on the border between two
 *    azimuths to the other one: such cells, and nothing else, may differ from the restatement.
 * 3. HITS.  Per point, the rasteriser's mapping px = (cf*x - sf*y) + txf, py = (sf*x + cf*y) + tyf and the IN GRID rule; every point that is
 *    IN GRID adds l_hit to its cell (an integer atomic: several points in one cell each add, in any order).
 * rr_occupancy_map[_device]: occ_u8 = clamp(128 + evidence, 0, 255) in integers.  128 is unknown, below it free, above it occupied;
 * rr_distance_field(occ, threshold 129 or more) takes it as it is.
 * The device forms enqueue on `stream` (NULL: the context's) with no host round trip and use NO context-owned memory: they may run on any
 * stream beside batches in flight.  rr_occupancy_update_device is three launches (profile, free space, hits, in that order: the free pass
 * writes without atomics), rr_occupancy_map_device one.  The host forms stage through context-owned buffers and are synchronous;
 * rr_occupancy_update reads evidence_i32 as well as writing it.
 * Refused with a message and nothing written: -1 for a null ctx; -2 for the update without a config (n_angles, n_cells, scroll_image,
 * theta_min, theta_inc and resolution are read); -3 for a null required buffer (d_points may be null with max_points 0), a grid or model
 * field outside its stated range, a non-finite cell, x0 or y0, a theta_inc of 0, n_frames outside 1..65535, max_points outside 0..65536,
 * states not 8-byte aligned, d_profile or d_evidence_i32 not 4-byte aligned.
 * LIMITS.  The map is planar.  One state per scan: a sweep's per-azimuth motion enters only through compensated points, the free pass
 * uses the scan's single state.  Free space ends at the FIRST detection of an azimuth; radar sees past it, the model does not.  Partial
 * azimuth coverage wraps as the Cartesian resampler's does.  No decay and no clamped log-odds inside the accumulator.  rr_multi has no
 * such call. */
typedef struct rr_occupancy_config {   /* 32 B */
    int32_t l_hit;           /* 1..127: evidence added per detection */
    int32_t l_free;          /* 0..127: evidence subtracted per free observation */
    int32_t margin_bins;     /* 0..n_cells: bins in front of an azimuth's first detection that stay unknown */
    int32_t max_free_bin;    /* 0..n_cells: free space is asserted for bins below it only; an azimuth with no detection is free up to it */
    int32_t reserved_[4];
} rr_occupancy_config;
int rr_occupancy_update_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_offsets /*[n][n_angles+1]*/, int n_frames,
                               int max_points, const double* d_states_or_NULL /*[n][4]*/, const rr_field_config* cfg,
                               const rr_occupancy_config* occ_cfg, float* d_profile /*[n][n_angles]*/,
                               int32_t* d_evidence_i32 /*[height][width]*/, void* stream);
int rr_occupancy_update(rr_ctx* ctx, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points,
                        const double* states_or_NULL, const rr_field_config* cfg, const rr_occupancy_config* occ_cfg,
                        int32_t* evidence_i32);                                                       /* host buffers, synchronous */
int rr_occupancy_map_device(rr_ctx* ctx, const int32_t* d_evidence_i32, const rr_field_config* cfg, uint8_t* d_occ_u8 /*[height][width]*/,
                            void* stream);
int rr_occupancy_map(rr_ctx* ctx, const int32_t* evidence_i32, const rr_field_config* cfg, uint8_t* occ_u8);   /* host buffers */
/* the blocking of k_occ_free: cells per workgroup, consecutive cells per thread, and the scans per staged profile chunk -- 0: the profile
 * is gathered, the scans are not chunked (tests put sizes at the edges) */
void rr_occupancy_tile_sizes(int* cells_per_group, int* cells_per_thread, int* scan_chunk);

/* ---- particle filter step: weigh, resample and move pose hypotheses (rr_filter.hip) ----------------------------------------
 * What stands between two calls of rr_score_poses when a pose is tracked over time: the records become weights, the weights are
 * systematically resampled, the survivors are moved by odometry plus diffusion.  Records, sums, ancestors and states stay in HBM.  The
 * reference has no such step: parity is UNPINNED and everything below is the build's own definition (a numpy restatement in
 * tests/filter_ref.py checks the kernels byte for byte).  Every result is an integer or a correctly rounded, un-fused f32 expression free
 * of trigonometry, and independent of order.
 * 1. rr_filter_resample[_device]: d_recs [n] (sum_d2 is read), a weight table uint16 [n_table] in HBM, n_out draws.
 *        dmin = min_i sum_d2[i]                                     best = the lowest i that holds it
 *        idx_i = min(n_table - 1, (sum_d2[i] - dmin) / quantum)     a u64 integer division
 *        w_i = table[idx_i]
 *        cum[i] = w_0 + ... + w_i   (u64, inclusive; an OUTPUT in the caller's buffer)        W = cum[n - 1] < 2^38        sum_w2 = sum w_i^2
 *        r = (phase * W) >> 24                                      t_j = (j * W + r) / n_out   in u64; j * W < 2^60
 *        ancestors[j] = min(n - 1, #{i : cum[i] <= t_j})            numpy's searchsorted(cum, t, side='right'), clamped
 *        n_unique = 1 + #{j >= 1 : ancestors[j] != ancestors[j - 1]}   (the ancestors are non-decreasing)
 *    The clamp also defines W == 0: every draw takes particle n - 1.  That is a definition, not an error.  The effective sample size
 *    is total_weight^2 / sum_w2, for the caller to take from the summary.
 * 2. rr_filter_move[_device]: d_states_in f32 [n][4] = (c, s, tx, ty), the convention of rr_score_poses; d_ancestors [n_out] or NULL,
 *    which means a = j (and needs n_out <= n); an ancestor past n - 1 is read as n - 1.  The odometry increment (Dc, Ds, dx, dy) is in the
 *    sensor frame and passed by value.  With mix32(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16 in uint32,
 *        key = mix32(seed ^ mix32(step))          and for draw j and k in 0, 1, 2:
 *        h = mix32(key ^ (8*j + 2*k))             g = mix32(key ^ (8*j + 2*k + 1))
 *        v_k = (h & 0xffff) + (h >> 16) + (g & 0xffff) + (g >> 16) - 131070
 *    an integer within +-131070, the centred sum of four uniforms, of variance (65536^2 - 1) / 3.  Then in f32, in exactly this order:
 *        (c, s, tx, ty) = states_in[a]
 *        nx = (float)v_0 * sigma_xy      ny = (float)v_1 * sigma_xy      t = (float)v_2 * sigma_t
 *        ux = dx + nx                    uy = dy + ny
 *        tx' = (c*ux - s*uy) + tx        ty' = (s*ux + c*uy) + ty
 *        q = t*t      den = 1.0f + q     nc = (1.0f - q) / den           ns = (t + t) / den
 *        rc = Dc*nc - Ds*ns              rs = Ds*nc + Dc*ns
 *        c1 = c*rc - s*rs                s1 = s*rc + c*rs
 *        m = sqrtf(c1*c1 + s1*s1)        c' = c1 / m                     s' = s1 / m
 *    with IEEE division and square root.  states_out [n_out][4] = (c', s', tx', ty') must not overlap states_in.  Non-finite values pass
 *    through (rr_score_poses costs a NaN state at count * cap2).
 * The device forms enqueue on `stream` (NULL: the context's) with no host round trip and use NO context-owned memory: cum is the scan's
 * only room.  rr_filter_resample_device is six launches (start values, minimum, tile sums, the scan of the tile sums by ONE workgroup,
 * cum, draws), none of which waits on another workgroup; rr_filter_move_device is one.  The host forms stage through context-owned
 * buffers and are synchronous.
 * Refused with a message and nothing written: -1 for a null ctx; -3 for a null required buffer or config, a config field outside its
 * stated range, reserved != 0, a non-finite or negative sigma, a non-finite increment, n or n_out outside 1..2^22, n_out > n without
 * ancestors, states that overlap or are not 16-byte aligned, d_recs, d_cum or d_summary not 8-byte aligned, d_ancestors not 4-byte or
 * d_table not 2-byte aligned.
 * LIMITS.  Planar.  One scan per step.  No adaptive particle count and no KLD sampling.  The noise is a sum of four uniforms, not a
 * Gaussian.  rr_multi has no such call. */
typedef struct rr_filter_config {   /* 32 B */
    uint32_t quantum;    /* 1..2^31: sum_d2 units per step of the weight table */
    uint32_t n_table;    /* 1..4096 */
    uint32_t phase;      /* 0..2^24 - 1: where the comb of draws starts */
    uint32_t seed;
    uint32_t step;       /* counter of this filter step; enters the hash */
    float    sigma_xy;   /* finite, >= 0: metres per unit of the integer variate */
    float    sigma_t;    /* finite, >= 0: tangent of the half angle per unit */
    uint32_t reserved;   /* must be 0 */
} rr_filter_config;
typedef struct rr_filter_summary {  /* 32 B */
    uint64_t min_sum_d2;
    uint64_t total_weight;
    uint64_t sum_w2;
    uint32_t best;       /* the lowest index that holds min_sum_d2 */
    uint32_t n_unique;   /* distinct ancestors among the n_out draws */
} rr_filter_summary;
int rr_filter_resample_device(rr_ctx* ctx, const rr_field_rec* d_recs /*[n]*/, int n /*1..2^22*/, const uint16_t* d_table /*[n_table]*/,
                              int n_out /*1..2^22*/, const rr_filter_config* cfg, uint64_t* d_cum /*[n]*/, uint32_t* d_ancestors /*[n_out]*/,
                              rr_filter_summary* d_summary, void* stream);
int rr_filter_resample(rr_ctx* ctx, const rr_field_rec* recs, int n, const uint16_t* table, int n_out, const rr_filter_config* cfg,
                       uint64_t* cum, uint32_t* ancestors, rr_filter_summary* summary);                 /* host buffers, synchronous */
int rr_filter_move_device(rr_ctx* ctx, const float* d_states_in /*[n][4]*/, int n, const uint32_t* d_ancestors_or_NULL /*[n_out]*/, int n_out,
                          float Dc, float Ds, float dx, float dy, const rr_filter_config* cfg, float* d_states_out /*[n_out][4]*/,
                          void* stream);
int rr_filter_move(rr_ctx* ctx, const float* states_in, int n, const uint32_t* ancestors_or_NULL, int n_out, float Dc, float Ds, float dx,
                   float dy, const rr_filter_config* cfg, float* states_out);                             /* host buffers, synchronous */
/* the blocking: records per scan tile (a workgroup's), draws per workgroup of the draw kernel, and the entries of cum a workgroup stages for
 * its draws -- 0: the draws search cum in global memory (tests put n at the edges) */
void rr_filter_tile_sizes(int* scan_tile, int* draws_per_group, int* search_tile);

/* ---- map refinement: nearest-cell transform and batched scan-to-map ICP (rr_refine.hip) -----------------------------------
 * What comes behind a lattice node or a particle: ONE observed scan is refined against the grid map from very many starting states at
 * once.  The map's nearest-cell (feature) transform is taken once; a hypothesis then costs one table look-up per point and iteration, and
 * all iterations run inside one launch.  The reference has no such step: parity is UNPINNED and everything below is the build's own
 * definition (a numpy restatement in tests/refine_ref.py checks the kernels byte for byte).  All f32 arithmetic is un-fused; every result is
 * an integer or a correctly rounded f64 expression without trigonometry.
 * Grid, IN GRID rule, cell index and pose convention are rr_field_config's and the likelihood field's (above), unchanged.
 * NONE = 0xFFFFFFFF, cap2 = max_dist^2.
 * 1. rr_nearest_field[_device]: (ctx, occ_u8, threshold 1..255, cfg, nearest_u32 [height][width], stream).
 *    A cell is occupied iff occ >= threshold, as in rr_distance_field.
 *    For cell (ix, iy), take over all occupied cells (jx, jy) the minimum of the 64-bit key (d2 << 32) | (jy * width + jx), with
 *    d2 = (ix-jx)^2 + (iy-jy)^2.  Ties in distance therefore go to the lowest linear index.
 *    nearest[iy][ix] is that linear index if the minimal d2 < cap2, else NONE.
 *    From this definition nearest != NONE exactly where rr_distance_field gives a value below cap2, and there d2(cell, nearest) equals
 *    that value.  nearest must not alias occ.
 * 2. rr_refine_poses[_device]: (ctx, points, d_count, max_points 0..65536, init f64 [n_hyp][4], n_hyp 1..2^22, nearest_u32, cfg,
 *    iterations 0..64, rr_icp_rec recs [n_hyp], stream).
 *    ONE scan is shared by all hypotheses.  Its count is read on the device and cut at max_points, which is flagged RR_ICP_TRUNCATED.
 *    Initial states are normalised exactly as rr_register_points does.  A state with no direction becomes the identity plus
 *    RR_ICP_DEGENERATE (in the host form too: nothing is refused for it).
 *    One pass at a state:
 *      Transform.   Round the state to f32.  px = (cf*x - sf*y) + txf, py = (sf*x + cf*y) + tyf, un-fused.
 *      Cell.        The IN GRID rule gives (ix, iy).
 *      Look-up.     k = nearest[iy*width+ix], jx = k % width, jy = k / width.
 *      Match test.  The point is MATCHED iff it is IN GRID, k != NONE and (ix-jx)^2 + (iy-jy)^2 <= cfg.gate^2.
 *      Quantise.    P = (int32)rintf(p * 256.0f) per coordinate.
 *      Target.      Q is the same quantisation of the nearest cell's centre: qx = x0 + ((float)jx + 0.5f) * cell, qy likewise.  This
 *                   is the occupancy grid's cell-centre expression.
 *    The eight int64 sums and the SOLVE are the scan matcher's, letter for letter: N, SPx, SPy, SQx, SQy, Sdot, Scross, Ssse; A, B, h; the
 *    degenerate rule; composition; renormalisation.
 *    The call runs `iterations` times (pass, solve).  Then one last pass writes sse and n_matched into the 48-byte rr_icp_rec.  The record
 *    type is reused.  iterations = 0 scores the states as they stand.  A state that holds a NaN in its translation leaves every point not
 *    IN GRID: N = 0, and every solve sets RR_ICP_DEGENERATE and keeps the state.
 *    To keep the scan matcher's overflow bound (|P|, |Q| <= 2^21), the call refuses with -3 a grid any of whose four extents is at or
 *    beyond 8192 m in magnitude.  The extents are x0, y0, x0 + width*cell and y0 + height*cell, taken in f64 from the f32 fields.
 * Other refusals follow the scan matcher and the likelihood field: null ctx -1; null buffers, ranges and alignment (8 bytes for init and
 * recs, 4 for nearest) -3.
 * The device forms enqueue on `stream` (NULL: the context's) with no host round trip: rr_nearest_field_device two launches (columns, rows),
 * rr_refine_poses_device ONE, whatever the iteration count.  They use NO context memory at all, so they run on any stream beside batches in
 * flight.  The host forms stage through context-owned buffers and are synchronous, with the count passed as a value. */
int rr_nearest_field_device(rr_ctx* ctx, const uint8_t* d_occ_u8, int threshold /*1..255*/, const rr_field_config* cfg,
                            uint32_t* d_nearest_u32 /*[height][width]*/, void* stream);
int rr_nearest_field(rr_ctx* ctx, const uint8_t* occ_u8, int threshold, const rr_field_config* cfg, uint32_t* nearest_u32);   /* host buffers */
int rr_refine_poses_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_count, int max_points,
                           const double* d_init /*[n_hyp][4]: c, s, tx, ty*/, int n_hyp /*1..2^22*/, const uint32_t* d_nearest_u32,
                           const rr_field_config* cfg, int iterations /*0..64*/, rr_icp_rec* d_recs /*[n_hyp]*/, void* stream);
int rr_refine_poses(rr_ctx* ctx, const rr_radar_point* points, uint32_t count, int max_points, const double* init, int n_hyp,
                    const uint32_t* nearest_u32, const rr_field_config* cfg, int iterations, rr_icp_rec* recs);   /* host buffers, synchronous */
/* the blocking of the kernels: points a wave of k_refine takes per step, hypotheses per workgroup of it, cells of a row per sweep of the
 * transform's row pass (tests put counts and sizes at their edges) */
void rr_refine_tile_sizes(int* points_tile, int* hyps_per_group, int* row_tile);

/* ---- beam model: the grid map cast at pose hypotheses, a scan's rays scored against it (rr_cast.hip) ------------------------
 * The complement of the likelihood field.  rr_score_poses looks only at where a scan's detections END; here every azimuth of a hypothesis
 * is cast through the map, and the range the map predicts is compared with the range the scan measured: rays that agree, rays that stop
 * short, rays that saw through a wall.  The same cast answers "what would a scan look like from here, according to the map".  The
 * reference has no such step: parity is UNPINNED and everything below is the build's own definition (a numpy restatement in
 * tests/cast_ref.py checks the kernels byte for byte).  All f32 arithmetic is un-fused; every result is an integer and independent of
 * order.
 * MAP.  A uint16 field exactly as rr_distance_field[_device] writes it, under its rr_field_config, whose IN GRID rule and cell index are
 * used unchanged; `gate` is ignored (any value passes).  A cell is OCCUPIED iff its field value is 0.  No occupancy bytes are passed.
 * DIRECTIONS.  dirs is float [n_angles][2], one (ca, sa) per azimuth INDEX a (not per image column), an input that is used as given: no
 * trigonometry on the device.
 * A RAY.  A hypothesis state (c, s, tx, ty) is f32, used as given with no normalisation, under the likelihood field's pose convention.
 * The ray of azimuth a is traced over the sample bins b = bin_begin + k * bin_step < bin_end, k = 0, 1, ...; all in f32, nothing fused:
 *     r = (float)(((double)b + 0.5) * resolution)          x = r * ca          y = r * sa
 *     px = (c*x - s*y) + tx          py = (s*x + c*y) + ty          then the IN GRID test and the cell index
 * The sample is a HIT iff it is IN GRID and its cell is OCCUPIED; a sample that is not IN GRID is not a hit and the march goes on.  The
 * expected bin e[a] is the smallest sampled b that is a hit, bin_end if there is none: a NaN anywhere gives bin_end.  That brute-force
 * march is the DEFINITION; the kernel skips samples the field value proves empty and must give the same e[a].
 * 1. rr_scan_profile[_device]: clouds as rr_detect_device writes them.  first_bin[f][a], uint16: with col the image column of azimuth a,
 *    the bin of the point at d_offsets[f][col] if the column has a detection (d_offsets[f][col + 1] > d_offsets[f][col]) and that index is
 *    below max_points, cut at n_cells; n_cells otherwise.  A plain kernel, a thread per (frame, azimuth).
 * 2. rr_cast_map[_device]: ranges[h][a] = e[a] of hypothesis h, uint16 [n_hyp][n_angles]: the expected scan of the map at each pose.
 * 3. rr_score_beams[_device]: ONE profile first_bin[n_angles], read on the device, against n_hyp hypotheses; one rr_beam_rec each.  Per
 *    azimuth, with m = first_bin[a]: an azimuth with m < bin_begin is left out and not counted in n_cast; m >= bin_end counts as "none".
 *        e none and m none: n_none          e none and m finite: n_open          e finite and m none: n_through
 *        both finite, d = m - e:   |d| <= tol_bins: n_agree      d < -tol_bins: n_short      d > tol_bins: n_through
 *                                  and in all three sum_abs += min(|d|, clip_bins)
 *    The five counts sum to n_cast.  Nothing of size n_hyp * n_angles is written.
 * n_angles, n_cells and resolution are the context's config's (-2 without one).  rr_set_config caps n_cells at 8192, so a bin always fits
 * the tables' 16 bits; the calls would refuse a config beyond 65535 (-3).
 * The device forms enqueue ONE launch on `stream` (NULL: the context's) with no host round trip, write only the caller's buffers and use
 * NO context-owned memory: they may run on any stream beside batches in flight.  The host forms stage through context-owned buffers and are
 * synchronous.
 * Refused with a message and nothing written: -1 for a null ctx; -2 without a config; -3 for a null required buffer or config, a grid
 * field but gate outside the likelihood field's ranges, a beam field outside its stated range, a non-zero reserved word, n_hyp outside its range
 * (1..65535 for rr_cast_map, 1..2^22 for rr_score_beams), n_frames outside 1..65535, max_points outside 0..65536, states or dirs not
 * 4-byte, the 16-bit tables not 2-byte or the records not 8-byte aligned.
 * LIMITS.  Planar.  First hit only: the map stops a ray where radar would see past.  One scan per rr_score_beams call.  No weight table
 * for rr_filter_resample, which takes rr_field_rec: mixing the two scores is the caller's.  rr_multi has no such call. */
typedef struct rr_beam_config {   /* 32 B */
    int32_t bin_begin, bin_end;   /* 0 <= bin_begin <= bin_end <= n_cells: the bins a ray samples */
    int32_t bin_step;             /* 1..64: every bin_step-th bin from bin_begin is a sample */
    int32_t tol_bins;             /* 0..n_cells: |m - e| within it is agreement */
    int32_t clip_bins;            /* 0..n_cells: what one azimuth adds to sum_abs at most */
    int32_t reserved_[3];         /* must be 0 */
} rr_beam_config;
typedef struct rr_beam_rec {   /* 32 B */
    uint32_t n_agree;     /* both finite, |m - e| <= tol_bins */
    uint32_t n_short;     /* both finite, the scan stopped more than tol_bins in front of the map's wall */
    uint32_t n_through;   /* the scan saw more than tol_bins past the map's wall, or saw nothing where the map has one */
    uint32_t n_open;      /* the scan has a detection where the map has nothing */
    uint32_t n_none;      /* neither has anything */
    uint32_t n_cast;      /* azimuths that took part: the sum of the five */
    uint64_t sum_abs;     /* sum over the azimuths with both finite of min(|m - e|, clip_bins) */
} rr_beam_rec;
int rr_scan_profile_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_offsets /*[n][n_angles+1]*/, int n_frames,
                           int max_points, uint16_t* d_first_bin /*[n][n_angles]*/, void* stream);
int rr_scan_profile(rr_ctx* ctx, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points,
                    uint16_t* first_bin);                                                             /* host buffers, synchronous */
int rr_cast_map_device(rr_ctx* ctx, const float* d_states /*[n_hyp][4]: c, s, tx, ty*/, int n_hyp /*1..65535*/,
                       const float* d_dirs /*[n_angles][2]*/, const uint16_t* d_field_u16, const rr_field_config* cfg,
                       const rr_beam_config* beam, uint16_t* d_ranges /*[n_hyp][n_angles]*/, void* stream);
int rr_cast_map(rr_ctx* ctx, const float* states, int n_hyp, const float* dirs, const uint16_t* field_u16, const rr_field_config* cfg,
                const rr_beam_config* beam, uint16_t* ranges);                                        /* host buffers, synchronous */
int rr_score_beams_device(rr_ctx* ctx, const uint16_t* d_first_bin /*[n_angles]*/, const float* d_states /*[n_hyp][4]*/,
                          int n_hyp /*1..2^22*/, const float* d_dirs /*[n_angles][2]*/, const uint16_t* d_field_u16,
                          const rr_field_config* cfg, const rr_beam_config* beam, rr_beam_rec* d_recs /*[n_hyp]*/, void* stream);
int rr_score_beams(rr_ctx* ctx, const uint16_t* first_bin, const float* states, int n_hyp, const float* dirs, const uint16_t* field_u16,
                   const rr_field_config* cfg, const rr_beam_config* beam, rr_beam_rec* recs);        /* host buffers, synchronous */
/* the blocking of k_cast: azimuths a wave takes per step (one per lane), hypotheses a wave takes in turn, hypotheses per workgroup
 * (tests put counts at the edges) */
void rr_cast_tile_sizes(int* angles_tile, int* hyps_per_wave, int* hyps_per_group);

/* ---- mesh maps: the scene's triangles sliced into the grid map (rr_slice.hip) -------------------------------------------------
 * The way from the mesh a context holds to the grid the map calls work on: every cell of an rr_field_config grid that some posed triangle
 * touches inside a height band [z_lo, z_hi] is marked, in the uint8 convention of rr_rasterize_points, so rr_distance_field,
 * rr_nearest_field and everything behind them take the result as it is.  A slice is geometry only: no occlusion, no visibility, no
 * materials.  The reference has no such step: parity is UNPINNED and everything below is the build's own definition (a numpy restatement in
 * tests/slice_ref.py checks the kernels byte for byte).  All f32 arithmetic is un-fused; every result is independent of order.
 * GEOMETRY.  The context's current scene: every face's rest corners moved by its object's pose, with the arithmetic of the dynamic scenes
 * (rr_set_object_poses).  What the context holds on the device is iterated: its triangle records; a face that the tree builders cut has
 * several records, which write the same values.  An empty mesh writes nothing and returns 0.
 * CELL SPACE.  A corner (x, y, z) has u = (x - x0) / cell and v = (y - y0) / cell, the grid's rule above; z stays in metres.  A record
 * with a u, v or z that is not finite is skipped.
 * BAND.  z_lo <= z_hi, both finite; z_lo == z_hi is a plane.  A record is rejected on the raw values, with no arithmetic, if
 * max(za, zb, zc) < z_lo or min(za, zb, zc) > z_hi.
 * CELL PREDICATE.  Cell (ix, iy) is marked by a record iff no axis of a separating-axis test separates the triangle in (u, v, z) from the
 * CLOSED box [ix, ix+1] x [iy, iy+1] x [z_lo, z_hi].  Touching counts as overlap: a reject needs a strict inequality that holds, so a NaN
 * (an overflowed product of huge coordinates) rejects nothing.  The axes, and the order of operations:
 *     box axes    z as under BAND; u: rejected iff max(u) < (float)ix or min(u) > (float)(ix + 1), on the raw values; v likewise
 *     per record  edges e0 = p1 - p0, e1 = p2 - p1, e2 = p0 - p2 from the RAW corners p_k = (u_k, v_k, z_k); the normal n = e0 x e1:
 *                 nu = e0v*e1z - e0z*e1v      nv = e0z*e1u - e0u*e1z      nz = e0u*e1v - e0v*e1u
 *                 cz = (z_lo + z_hi) * 0.5f   hz = (z_hi - z_lo) * 0.5f   and for a cell hu = hv = 0.5f
 *     per cell    the corners are centred on the cell first: c_k = (u_k - (ix + 0.5f), v_k - (iy + 0.5f), z_k - cz); then the products
 *     normal      d = (nu*c0u + nv*c0v) + nz*c0z      r = (hu*|nu| + hv*|nv|) + hz*|nz|      rejected iff d > r or d < -r
 *     edge j      against the corners a = c_j and b = c_(j+2) (the third projects as a does); with e = e_j, each rejected iff both
 *                 projections are > r or both are < -r:
 *                 (1,0,0) x e:   ez*av - ev*az,  ez*bv - ev*bz      r = hv*|ez| + hz*|ev|
 *                 (0,1,0) x e:   eu*az - ez*au,  eu*bz - ez*bu      r = hu*|ez| + hz*|eu|
 *                 (0,0,1) x e:   ev*au - eu*av,  ev*bu - eu*bv      r = hu*|ev| + hv*|eu|
 * An axis that vanishes (a zero-area or collinear triangle) gives 0 > 0: it rejects nothing and the other axes decide.
 * CANDIDATE CELLS.  The u and v box axes pass exactly for ix in ceil(min u) - 1 .. floor(max u) and iy likewise (the closed box of the cell
 * below an integer minimum touches it), clamped to the grid in float before any conversion to int.  The definition is the predicate over
 * EVERY cell of the grid; the kernels walk the candidates only, and their tile prefilter never drops a cell the predicate marks (DESIGN.md
 * §28).
 * OUTPUTS.  d_occ_u8[iy][ix] = 1 for every marked cell: ones only, into a buffer that the caller zeroed or that already holds a map, so
 * the call composes with rr_rasterize_points and with several bands or calls in any order.  With d_object_u32: d_object_u32[iy][ix] =
 * min(what it held, object id) over all records that mark the cell; the caller fills it with 0xFFFFFFFF.  d_skip_u8 [n_objects]: a
 * non-zero byte leaves that object's records out entirely (a static prior map without the parked and moving objects).
 * The device form enqueues on `stream` (NULL: the context's) with no host round trip: a 4-byte memset and two launches.  It reads the scene
 * the context holds when the kernels run, so the CALLER orders it against rr_set_mesh*, rr_set_object_poses, rr_update_vertices and
 * rr_rebuild_tree (they drain the device before they change it; a slice must not be enqueued while one of them runs).  It uses
 * context-owned scratch, one set per stream the call has been made on (a list of one word per record; growing it drains that stream):
 * calls on different streams may overlap.  The host form
 * stages through context-owned buffers, is synchronous and ACCUMULATES: it reads occ_u8 and object_u32 as well as writing them.
 * Refused with a message and nothing written: -1 for a null ctx; -2 when no mesh has been set; -3 for a null config, grid or d_occ_u8, a
 * grid field outside rr_field_config's stated ranges, z_lo or z_hi not finite or z_lo > z_hi, flags != 0, or a d_object_u32 that is not
 * 4-byte aligned.
 * LIMITS.  A cell column is marked or not: no coverage fraction, no 3-D voxels.  rr_multi has no such call. */
typedef struct rr_slice_config {   /* 16 B */
    float    z_lo, z_hi;   /* the band in metres, map frame: finite, z_lo <= z_hi */
    uint32_t flags;        /* must be 0 */
    int32_t  reserved_;
} rr_slice_config;
int rr_slice_mesh_device(rr_ctx* ctx, const rr_slice_config* slice, const rr_field_config* cfg, const uint8_t* d_skip_u8_or_NULL /*[n_objects]*/,
                         uint8_t* d_occ_u8 /*[height][width]*/, uint32_t* d_object_u32_or_NULL /*[height][width]*/, void* stream);
int rr_slice_mesh(rr_ctx* ctx, const rr_slice_config* slice, const rr_field_config* cfg, const uint8_t* skip_u8_or_NULL, uint8_t* occ_u8,
                  uint32_t* object_u32_or_NULL);                                        /* host buffers, synchronous, accumulating */
/* the blocking of the kernels: the largest candidate box (in cells) a record's own thread tests, the side of a tile of k_slice_large, the
 * threads of a workgroup of either kernel (tests put boxes, grid sides and record counts at the edges) */
void rr_slice_tile_sizes(int* small_cells, int* tile_side, int* group_size);

/* ---- connected components: the clusters of polar images, the segments of grid maps (rr_components.hip) ------------------------------
 * The step between "pixels" and "things": the foreground of a thresholded uint8 plane grouped into its connected components, as a label
 * plane, a cleaned plane and one record per component.  One primitive serves the returns of a polar image (a cylinder: the column axis may
 * wrap) and the occupied cells of a grid map (small components dropped before the map goes on to rr_distance_field, rr_nearest_field or
 * rr_cast_map).  The reference has no such step: parity is UNPINNED and everything below is the build's own definition (a numpy restatement
 * in tests/components_ref.py checks the kernels byte for byte).  Integers only; every result is independent of order.
 * INPUT.  uint8 planes [n][height][width], row-major.  A pixel is foreground iff value >= threshold.  Two foreground pixels are neighbours
 * iff they differ by one in row or column (connectivity 4) or by at most one in both (connectivity 8).  With wrap_x, column width-1 is also
 * the left neighbour of column 0, diagonally as well under connectivity 8.  Rows never wrap; planes never touch each other.
 * DEFINITION.  A component is a class of the transitive closure of "neighbours".  The LABEL of a foreground pixel is the linear index
 * row * width + col of the smallest-index pixel of its component (the component's root); background is RR_LABEL_NONE.  A component with
 * fewer than min_pixels pixels is DROPPED: its pixels read RR_LABEL_NONE as well and are 0 in the cleaned plane, which keeps the input's
 * value under every kept pixel.  Kept components are listed in ascending root order; a component's id is its index in that list
 * (a binary search of the roots for a label gives it).
 * RECORDS.  For each plane the first min(kept, max_components) records in root order are written, every byte of them, and nothing beyond:
 * the convention of rr_detect_device's offsets.  d_counts [n][2] holds the TRUE number of kept components (also past max_components) and
 * the number of dropped ones.  row_min .. col_max are the plain extents.  col_lo_max is the largest occupied column < width / 2, col_hi_min
 * the smallest occupied column >= width / 2, each RR_LABEL_NONE if there is none: with RR_COMP_SEAM they give the circular arc of a seam
 * component narrower than half the circle, col_hi_min .. width-1, 0 .. col_lo_max.  All four column fields, the row extents, the flags and
 * the peak are order-independent min / max / or values, the counts and sums integer sums.  peak is the largest plane value in the
 * component, at (peak_row, peak_col); ties go to the lower linear index.  The sums run over the component's pixels in plain row and column
 * coordinates (a seam component's centroid is the caller's to unwrap).
 * The device form enqueues on `stream` (NULL: the context's): eight launches, no memset, no host round trip, no workgroup waiting for
 * another.  All working memory is the caller's d_scratch (rr_components_scratch_bytes; its contents before the call do not matter, and
 * the next call may have another shape): no context memory, so calls may run on any stream beside batches in flight.  The link plane of the
 * union-find is d_labels when one is given.  The cleaned plane must not overlap the input.  The host form stages through context-owned
 * buffers and is synchronous.  No config or mesh is needed in the context: the shape comes with the call.
 * Refused with a message and nothing written: -1 for a null ctx; -3 for a null planes, config, counts or scratch buffer, n_planes outside
 * 1..65535, a config field outside its stated range or reserved_ != 0, wrap_x with width < 3, records or scratch that are not 16-byte
 * aligned, scratch_bytes below rr_components_scratch_bytes, d_comps given with max_components == 0 or missing with max_components > 0, a
 * cleaned plane that overlaps the input.
 * LIMITS.  No neighbourhood wider than 8 (bridging gaps between sparse detections is a dilation the caller does first); no dense ids in the
 * label plane; 2-D only.  rr_multi has no such call. */
typedef struct rr_components_config {   /* 32 B */
    int32_t height, width;     /* 1..8192 each */
    int32_t threshold;         /* 1..255: foreground iff value >= threshold */
    int32_t connectivity;      /* 4 or 8 */
    int32_t wrap_x;            /* 0 | 1; 1 needs width >= 3 */
    int32_t min_pixels;        /* >= 1: smaller components are dropped */
    int32_t max_components;    /* >= 0: records written per plane; 0 counts only */
    int32_t reserved_;         /* 0 */
} rr_components_config;

#define RR_COMP_SEAM   1u   /* holds two neighbouring pixels across the wrap seam */
#define RR_COMP_BORDER 2u   /* touches row 0 or H-1, or (wrap_x == 0) column 0 or W-1 */
typedef struct rr_component {           /* 80 B, five 16-B stores, every byte written */
    uint32_t root, n_pixels, row_min, row_max;
    uint32_t col_min, col_max, col_lo_max, col_hi_min;
    uint32_t peak, peak_row, peak_col, flags;
    uint64_t sum_intensity, sum_row;
    uint64_t sum_col, reserved_;
} rr_component;

size_t rr_components_scratch_bytes(int n_planes, const rr_components_config* cfg);   /* 0 for a refused shape */
/* the tile of the first kernel, in pixels (tests put shapes, bridges and chains at its borders) */
void   rr_components_tile_sizes(int* tile_w, int* tile_h);
int rr_label_components_device(rr_ctx* ctx, const uint8_t* d_planes_u8, int n_planes, const rr_components_config* cfg,
        uint32_t* d_labels_or_NULL /*[n][H][W]*/, uint8_t* d_clean_u8_or_NULL /*[n][H][W]*/,
        rr_component* d_comps /*[n][max_components], NULL iff max_components == 0*/,
        uint32_t* d_counts /*[n][2]: kept (TRUE total, also past max_components), dropped*/,
        void* d_scratch, size_t scratch_bytes, void* stream);
int rr_label_components(rr_ctx* ctx, const uint8_t* planes_u8, int n_planes, const rr_components_config* cfg,
        uint32_t* labels_or_NULL, uint8_t* clean_u8_or_NULL, rr_component* comps, uint32_t* counts);   /* host, synchronous */

/* ---- correlative scan matching: exact pyramid search of the likelihood field (rr_correlate.hip) -----------------------------------
 * The search over a WIDE pose window that stands between place recognition (a coarse candidate) and rr_refine_poses / rr_register_points
 * (a guess within a few cells): one scan, n_rot yaws, every whole-cell translation of a window of up to +-2047 cells.  A min-pyramid of
 * the distance field bounds every block of translations from below, so almost all of the window is never visited; on whole-cell offsets
 * the pruning is EXACT: the result is the argmin an exhaustive search of the same nodes gives, byte for byte.  The reference has no such
 * step: parity is UNPINNED and everything below is the build's own definition (a numpy restatement in tests/correlate_ref.py checks the
 * kernels byte for byte).  All f32 arithmetic is un-fused; every result is an integer and independent of order.
 * INPUTS.  One scan, d_points[0 .. min(*d_count, max_points)), the count read on the device, max_points 0..65536.  A field uint16
 * [height][width] exactly as rr_distance_field writes it (every value <= cap2 = max_dist * max_dist) under its rr_field_config, as plane 0
 * of a pyramid.  n_rot in 1..4096 ANCHOR states f32 (c, s, tx, ty), used as given: each places the scan at the centre of the window under
 * one yaw.  An rr_corr_config.  The call is refused if n_rot * (2*half_x+1) * (2*half_y+1) >= 2^31.
 * ANCHORED CELL.  For rotation r and point i: px, py by the likelihood field's mapping in un-fused f32; u = (px - x0) / cell, v likewise.
 * The point is USABLE iff u and v are finite and |u|, |v| < 16384; then bx = (int)floorf(u), by = (int)floorf(v), which may be negative or
 * beyond the grid.  An unusable point costs cap2 at every node.
 * SCORE.  F(x, y) = field[y][x] inside the grid, cap2 outside.  score(r, dx, dy) = sum over ALL points of F(bx + dx, by + dy) for
 * |dx| <= half_x, |dy| <= half_y.  At (dx, dy) = (0, 0) this is exactly rr_score_poses's sum_d2 for the anchor state.  THE DIFFERENCE:
 * any other offset moves the ANCHORED CELL by whole cells; it is not the metric state (tx + dx * cell, ty + dy * cell) rounded again,
 * which rr_score_poses would put through the division once more and may land a point one cell aside.  That is what makes the bound exact.
 * The node index is (r * (2*half_y+1) + dy + half_y) * (2*half_x+1) + dx + half_x; the result is the node of smallest (score, index).
 * PYRAMID.  rr_field_pyramid[_device] writes levels + 1 planes [height][width] uint16: plane 0 is the field, P_h[y][x] the minimum over
 * 0 <= a, b < 2^h of F(x + a, y + b), built level from level (four reads at stride 2^(h-1), cap2 beyond the edge).  d_pyramid_u16 may be
 * d_field_u16 itself (a field computed into the head of the pyramid's buffer: plane 0 is then left as it is); any other overlap is the
 * caller's error.  A pyramid of more levels than a search uses serves it as well.
 * LOOK-UP.  Q_h(x, y) for any integers: cap2 if x >= width, y >= height, x + 2^h <= 0 or y + 2^h <= 0; otherwise P_h[max(y,0)][max(x,0)]
 * (a clamped window is a superset of the clipped one: still a lower bound).
 * CANDIDATES.  (r, ox, oy) at level h covers dx in [ox, ox + 2^h) and dy likewise, clipped to the window; its bound is
 * LB = sum over the points of Q_h(bx + ox, by + oy), cap2 for an unusable point.  The top-level candidates start at -half + j * 2^levels;
 * children are the four offsets at stride 2^(h-1), those that start beyond half_x or half_y dropped.
 * SEARCH, deterministic.  1. Greedy descent: the top-level candidate of smallest (LB, r, oy, ox), of its children the smallest again, down
 * to level 0; U is that node's exact score.  2. Level-synchronous pruning with that fixed U: a candidate survives iff LB <= U (ties reach
 * level 0), survivors are expanded, at level 0 the bound is the score.  3. The winner is the smallest packed key score << 31 | index
 * (score < 2^33).  levels = 0 evaluates every node: the exhaustive search in the same code.
 * OVERFLOW.  If the survivors of a level h >= 1 exceed `capacity`, the record is the greedy node with RR_CORR_OVERFLOW set; nothing
 * further is examined; kept[h] holds the true count, the counts of the levels below are 0.  Survivor counts do not depend on order, so
 * the outcome is deterministic.  Level 0 keeps no list and cannot overflow.
 * RECORD.  evaluated[h] and kept[h] are the bounds computed and the survivors at level h in step 2 (the descent's own 4 * levels bounds
 * and the first pass over the top level, which finds its start, are not counted; entries above `levels` are 0).
 * The device forms enqueue on `stream` (NULL: the context's) with no host round trip: rr_field_pyramid_device levels + 1 launches (levels
 * when plane 0 is in place), rr_correlate_scan_device levels + 5 (cells, top, descent, top again, one per level below the top sized by
 * `capacity` with the live count read on the device, finish).  No workgroup waits for another.  All working memory is the caller's
 * d_scratch (rr_correlate_scratch_bytes; its contents before the call do not matter): no context memory, so calls may run on any stream
 * beside batches in flight, each call with a scratch of its own.  The host forms stage through context-owned buffers and are synchronous.
 * Refused with a message and nothing written: -1 for a null ctx; -3 for a null required buffer or config, a grid field outside
 * rr_field_config's stated ranges, a search field outside its stated range or a non-zero reserved word, max_points outside 0..65536,
 * n_rot outside 1..4096, 2^31 nodes or more, d_rot not 4-byte, the pyramid not 2-byte, the record or the scratch not 16-byte aligned,
 * scratch_bytes below rr_correlate_scratch_bytes.  rr_multi has no such call. */
typedef struct rr_corr_config {   /* 32 B */
    int32_t half_x, half_y;    /* 0..2047 cells: the window is |dx| <= half_x, |dy| <= half_y */
    int32_t levels;            /* 0..8: the top-level candidates are 2^levels cells wide; 0 is the exhaustive search */
    int32_t capacity;          /* 1..2^24: candidates per list */
    int32_t reserved_[4];      /* 0 */
} rr_corr_config;

#define RR_CORR_OVERFLOW 1u   /* a level's survivors exceeded capacity: the record is the greedy node */
typedef struct rr_corr_rec {     /* 112 B, seven 16-B stores, every byte written */
    int32_t  rot, dx, dy;      /* the winner: its anchor state and its offset in cells */
    uint32_t flags;
    uint64_t sum_d2;           /* of the winner, as in rr_field_rec: its score */
    uint32_t n_in, n_hit;      /* of the winner, as in rr_field_rec */
    uint64_t upper;            /* U, the greedy node's score */
    uint32_t evaluated[9];     /* bounds computed per level */
    uint32_t kept[9];          /* survivors per level */
} rr_corr_rec;

size_t rr_correlate_scratch_bytes(int n_rot, int max_points, const rr_corr_config* cfg);   /* 0 for a refused shape */
/* the blocking of the kernels: points a wave takes per step, top-level candidates of one row per wave of k_corr_top, parents per wave of
 * k_corr_expand (tests put counts and windows at their edges) */
void   rr_correlate_tile_sizes(int* points_tile, int* tops_per_wave, int* parents_per_wave);
int rr_field_pyramid_device(rr_ctx* ctx, const uint16_t* d_field_u16 /*[height][width]*/, const rr_field_config* cfg, int levels /*0..8*/,
                            uint16_t* d_pyramid_u16 /*[levels+1][height][width]*/, void* stream);
int rr_field_pyramid(rr_ctx* ctx, const uint16_t* field_u16, const rr_field_config* cfg, int levels, uint16_t* pyramid_u16);   /* host buffers */
int rr_correlate_scan_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_count, int max_points,
                             const float* d_rot /*[n_rot][4]: c, s, tx, ty*/, int n_rot /*1..4096*/,
                             const uint16_t* d_pyramid_u16 /*[levels+1][height][width]*/, const rr_field_config* cfg, const rr_corr_config* corr,
                             rr_corr_rec* d_rec /*one record*/, void* d_scratch, size_t scratch_bytes, void* stream);
int rr_correlate_scan(rr_ctx* ctx, const rr_radar_point* points, uint32_t count, int max_points, const float* rot, int n_rot,
                      const uint16_t* pyramid_u16, const rr_field_config* cfg, const rr_corr_config* corr,
                      rr_corr_rec* rec);                                                  /* host buffers, synchronous */

/* ---- oriented surface points and point-to-line scan matching (rr_surfels.hip) ----------------------------------------------------
 * What rr_register_points lacks: a detected cloud reduced to a sparse set of ORIENTED SURFACE POINTS (a local mean with a normal taken
 * from the local scatter), and a batched matcher whose residual is only the distance component ALONG that normal, so a cloud no longer
 * slides along a sparsely sampled wall.  The reference has no such step: parity is UNPINNED and everything below is the build's own
 * definition (a numpy restatement in tests/surfels_ref.py checks the kernels byte for byte).  Integer sums, f64 steps of + - * / sqrt
 * without trigonometry, a fixed iteration count; all f32 arithmetic is un-fused.
 *
 * 1. rr_surface_points[_device]: n clouds -> oriented surface points.  The clouds are laid out as rr_detect_device /
 *    rr_compensate_points_device write them; the count of frame f is min(d_offsets[f][n_angles], max_points), read on the device; a cut
 *    count sets RR_SURFELS_TRUNCATED.  z, intensity, column and bin are ignored.  With cell_q = (int32)rintf(cell * 256.0f) (1..4096):
 *    QUANTISE.  A point is a candidate iff x and y are finite and below 8192 in magnitude; X = (int32)rintf(x * 256.0f), Y likewise.
 *    CELL.  half = (width * cell_q) / 2 (integer division); U = X + half, V = Y + half; ix = floor(U / cell_q), iy = floor(V / cell_q)
 *    (FLOOR, not truncation: U may be negative); the point is dropped unless 0 <= ix, iy < width.  The linear cell index is
 *    iy * width + ix.  Coordinates RELATIVE to the cell's own origin: rx = U - ix * cell_q, ry = V - iy * cell_q, both in [0, cell_q).
 *    PER-CELL SUMS.  Six int64 sums per cell over its points: N, Sx = sum rx, Sy = sum ry, Sxx = sum rx*rx, Sxy = sum rx*ry, Syy = sum ry*ry.
 *    SAMPLE.  A surface point exists for each cell that holds at least one point itself; its sample is every point of the 3 x 3 block
 *    of cells around it, clipped at the grid edge.  The sums of the neighbour at (ix + a, iy + b), a, b in -1..1, are shifted to the
 *    centre cell's origin exactly, with ox = a * cell_q, oy = b * cell_q:
 *        Sx + N*ox      Sy + N*oy      Sxx + 2*ox*Sx + N*ox*ox      Sxy + ox*Sy + oy*Sx + N*ox*oy      Syy + 2*oy*Sy + N*oy*oy
 *    and added up; N, Sx .. Syy below are those totals.
 *    SCATTER, exact int64:  Cxx = N*Sxx - Sx*Sx    Cxy = N*Sxy - Sx*Sy    Cyy = N*Syy - Sy*Sy.
 *    PROOF.  A shifted coordinate lies in [-cell_q, 2*cell_q), so it is below 2^13 in magnitude; N <= 65536 = 2^16 (a frame has no more
 *    points).  So |Sx| <= 2^29, Sxx <= 2^42, N*Sxx <= 2^58 and Sx*Sx <= 2^58: every product stays below 2^59, every scatter entry
 *    within +-2^59, and T, d, o below within +-2^60.
 *    EIGEN STEP, f64, + - * / sqrt only, evaluated as written.  T = Cxx + Cyy, d = Cxx - Cyy, o = 2*Cxy as int64, each converted to f64:
 *        h = sqrt(d*d + o*o)     lmax = (T + h) / 2     v = (T - h) / 2, lmin = v if v > 0, else 0
 *        the tangent (tx, ty) is (h + d, o) if d >= 0, else (o, h - d), each divided by sqrt(tx*tx + ty*ty)
 *        the mean in quantised units: mx = (double)(ix*cell_q - half) + (double)Sx / (double)N, my likewise
 *        the normal is (-ty, tx), negated iff nx*mx + ny*my > 0: normals face the sensor at the origin
 *    KEEP the surface point iff N >= min_points, h > 0 and lmin <= (double)max_ratio * lmax.  (h == 0: one repeated point, or a
 *    sample with no direction, as the corners of a square.)
 *    RECORD.  x = (float)(mx / 256.0), y likewise; nx, ny rounded to f32; with den = ((double)N * (double)N) * 65536.0,
 *    var_n = (float)(lmin / den), var_t = (float)(lmax / den): the variance across and along the surface in m^2; count = N; cell.
 *    OUTPUT.  Per frame the first min(kept, max_surfels) records in ascending cell order, every byte of them, and nothing beyond; no
 *    execution order can change a byte.  d_counts [n][2] holds the TRUE number kept (also past max_surfels) and the flags
 *    (RR_SURFELS_TRUNCATED; RR_SURFELS_CAPPED: kept > max_surfels): the convention of rr_label_components.
 *    The device form enqueues on `stream` (NULL: the context's) a memset of the sums and four launches: bin (one 64-bit integer vector
 *    atomic per sum into the point's own cell), gather-and-decide (a launch of its own: the launch boundary makes the sums visible; per
 *    chunk of cells the number kept), the scan of the chunks by one workgroup per frame, and write.  No host round trip, no workgroup
 *    waiting for another.  All working memory is the caller's d_scratch (rr_surfels_scratch_bytes: 48 bytes of sums and one flag byte
 *    per cell and frame, and the scan's partials; its contents before the call do not matter): no context memory, so calls may run on
 *    any stream beside batches in flight.  The host form stages through context-owned buffers and is synchronous.
 *    Refused with a message and nothing written: -1 for a null ctx; -2 without a config (n_angles is the offsets' stride); -3 for a
 *    null required buffer or config, n_frames outside 1..65535, max_points outside 0..65536, max_surfels outside 0..2^20, a config
 *    field outside its stated range or a non-zero reserved word, records or scratch that are not 16-byte aligned, counts that are not
 *    4-byte aligned, d_surfels given with max_surfels == 0 or missing with max_surfels > 0, scratch_bytes below rr_surfels_scratch_bytes.
 *
 * 2. rr_register_surfels[_device]: n source clouds registered against ONE target of surface points by point-to-line ICP with a FIXED
 *    iteration count.  The call shape, the state (c, s, tx, ty) in f64, d_init and its normalisation, the flags, the record and d_corr
 *    are those of rr_register_points_device; the target is d_tgt_surfels[0 .. min(*d_tgt_count, max_tgt)), the count a device uint32_t*
 *    (a caller passes &counts[g][0] of rr_surface_points_device with max_tgt = its max_surfels).
 *    One CORRESPONDENCE PASS is steps 1 to 3 of rr_register_points with the surfels' means (x, y) as the target and a range limit of
 *    2048 in place of 8192: ascending walk, strict d2 < best (ties go to the lower index, a NaN never wins), matched iff px and py are
 *    finite and below 2048 in magnitude, j* != NONE and best <= gate2.  A target surfel is a candidate iff x and y are finite and below
 *    2048 in magnitude AND nx and ny are finite and at most 1 in magnitude.
 *    SUMS.  For a matched pair: P = (int32)rintf(p * 64.0f) per coordinate of the moved point, Q likewise from the surfel's mean,
 *    M = (int32)rintf(n * 1024.0f) per coordinate of its normal.  e = P - Q, r = Mx*ex + My*ey, a = (Px*My - Py*Mx, Mx, My).
 *    BOUNDS.  |P|, |Q| <= 2^17, |M| <= 2^10, |e| <= 2^18, so |r| <= 2^29, |a0| <= 2^28, |a1|, |a2| <= 2^10.  Per term and, over at
 *    most 65,536 = 2^16 pairs, per sum:
 *        a0*a0 <= 2^56 (sum 2^72)   a0*r <= 2^57 (sum 2^73)   r*r <= 2^58 (sum 2^74): TWO LIMBS each
 *        a0*a1, a0*a2 <= 2^38 (2^54)   a1*r, a2*r <= 2^39 (2^55)   a1*a1, a1*a2, a2*a2 <= 2^20 (2^36)   N <= 2^16: one int64 each
 *    A two-limb term T is split BEFORE any reduction as lo = T & 0xFFFFFFFF (0 .. 2^32-1, its sum below 2^48) and hi = T >> 32
 *    (arithmetic, |hi| <= 2^26, its sum within +-2^42); the solve recombines (double)hi * 4294967296.0 + (double)lo.  So the fourteen
 *    int64 sums per frame are N, H00lo, H00hi, H01, H02, H11, H12, H22, g0lo, g0hi, g1, g2, rrlo, rrhi (H = sum a a^T, g = sum a*r),
 *    all exact integers: the result is independent of order.
 *    One SOLVE is f64, + - * / only but for the closing sqrt of rr_register_points' renormalisation, evaluated as written.  H delta = -g
 *    by an explicit LDL^T:
 *        d0 = H00                              l10 = H01/d0    l20 = H02/d0
 *        d1 = H11 - l10*H01                    m21 = H12 - l20*H01    l21 = m21/d1
 *        d2 = (H22 - l20*H02) - l21*m21
 *        z0 = -g0    z1 = -g1 - l10*z0    z2 = (-g2 - l20*z0) - l21*z1
 *        x2 = z2/d2    x1 = z1/d1 - l21*x2    x0 = (z0/d0 - l10*x1) - l20*x2
 *    if N < 3 or a pivot d0, d1, d2 is not > 0 (tested as each is formed): flags |= RR_ICP_DEGENERATE and the state keeps its value
 *    in this iteration.  Else theta = x0 (radians: the units cancel), dtx = x1 / 64, dty = x2 / 64, and the turn by Cayley:
 *        u = theta/2    dc = (1 - u*u) / (1 + u*u)    ds = (2*u) / (1 + u*u)
 *    composed onto the state and renormalised exactly as rr_register_points does (c', s', tx', ty' from dc, ds, dtx, dty).
 *    The call runs `iterations` times (pass, solve), then one last pass.  The record: the state, n_matched = N, flags, and
 *    sse = rrhi * 2^32 + rrlo in (1/65536 m)^2 (r is in 1/64 m times 1/1024), saturated to INT64_MAX if rrhi >= 2^30.
 *    The device form enqueues 2 * iterations + 3 launches with no host round trip and touches no context memory but a scratch
 *    accumulator of 112 bytes per frame kept PER STREAM, as rr_register_points_device does; d_init and d_recs must be 8-byte, the
 *    target 16-byte aligned.  Refusals are those of rr_register_points[_device].
 *    LIMITS.  No surfel-to-surfel matching, no weights beyond the gate.  A corridor whose normals are all parallel leaves H singular:
 *    for normals along an axis or a diagonal a pivot is exactly 0 and the frame is DEGENERATE; for a general direction the rounding
 *    of the pivots decides.  rr_multi has no such call. */
typedef struct rr_surfel_config {   /* 32 B */
    float   cell;              /* metres; cell_q = rintf(cell * 256) in 1..4096 */
    int32_t width;             /* 1..1024 cells per side of a square grid centred on the sensor origin */
    int32_t min_points;        /* 2..65536: fewest points of a sample */
    float   max_ratio;         /* 0..1: largest lmin / lmax */
    int32_t reserved_[4];      /* 0 */
} rr_surfel_config;

#define RR_SURFELS_TRUNCATED 1u   /* the frame's count exceeded max_points: the cloud was cut */
#define RR_SURFELS_CAPPED    2u   /* more surface points were kept than max_surfels: the first max_surfels were written */
typedef struct rr_surfel {     /* 32 B, two 16-B stores, every byte written */
    float x, y;                /* the sample's mean, metres */
    float nx, ny;              /* the unit normal, facing the origin */
    float var_n, var_t;        /* variance across and along the surface, m^2 */
    uint32_t count;            /* N of the sample */
    uint32_t cell;             /* linear cell index iy * width + ix */
} rr_surfel;

size_t rr_surfels_scratch_bytes(int n_frames, const rr_surfel_config* cfg);   /* 0 for a refused shape */
/* the blocking of the kernels: points per workgroup of the binning launch, cells per chunk of the scan (tests put counts at their edges) */
void   rr_surfels_tile_sizes(int* points_tile, int* cells_chunk);
int rr_surface_points_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_offsets /*[n][n_angles+1]*/, int n_frames,
                             int max_points, const rr_surfel_config* cfg, rr_surfel* d_surfels /*[n][max_surfels], NULL iff max_surfels == 0*/,
                             int max_surfels, uint32_t* d_counts /*[n][2]: kept (TRUE total), flags*/, void* d_scratch, size_t scratch_bytes,
                             void* stream);
int rr_surface_points(rr_ctx* ctx, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points,
                      const rr_surfel_config* cfg, rr_surfel* surfels, int max_surfels, uint32_t* counts);   /* host buffers, synchronous */
int rr_register_surfels_device(rr_ctx* ctx, const rr_radar_point* d_points, const uint32_t* d_offsets /*[n][n_angles+1]*/, int n_frames,
                               int max_points, const rr_surfel* d_tgt_surfels, const uint32_t* d_tgt_count, int max_tgt,
                               const double* d_init_or_NULL /*[n][4]*/, float gate, int iterations /*0..64*/, rr_icp_rec* d_recs /*[n]*/,
                               uint32_t* d_corr_or_NULL /*[n][max_points]*/, void* stream);
int rr_register_surfels(rr_ctx* ctx, const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points,
                        const rr_surfel* tgt_surfels, uint32_t tgt_count, int max_tgt, const double* init_or_NULL, float gate, int iterations,
                        rr_icp_rec* recs, uint32_t* corr_or_NULL);                       /* host buffers, synchronous */

/* ---- pose-graph optimisation: batched SE(2) Gauss-Newton with preconditioned conjugate gradients (rr_graph.hip) -----------------
 * The back end behind the matchers: N rigid 2-D states tied by E relative measurements (an odometry chain and its loop closures) are made
 * consistent, and the result is the pose table the map calls take.  The reference has no such step: parity is UNPINNED and everything below
 * is the build's own definition (a numpy restatement in tests/graph_ref.py checks the kernels byte for byte).  All arithmetic is f64,
 * + - * / sqrt only, un-fused and evaluated as written; every sum has a stated order; no atomic takes part in the arithmetic.
 * OUT OF SCOPE: full 3 x 3 information matrices (an edge carries two weights), 3-D poses, incremental re-solves, marginal covariances.
 *
 * NODES.  states f64 [N][4] = (c, s, tx, ty), the layout of rr_icp_rec's state, taken as given (a caller passes a unit (c, s)); one byte
 * per node, non-zero: the node is FIXED.  EDGES.  rr_graph_edge: (c, s, tx, ty) is the measured state of node j in node i's frame -- a
 * record of rr_register_points, rr_register_surfels or rr_refine_poses with target scan i and source scan j, as it comes.
 * RESIDUAL of an edge, with (ci, si, txi, tyi) and (cj, sj, txj, tyj) the states of its nodes and z the measurement:
 *     dx = txj - txi    dy = tyj - tyi    ux = ci*dx + si*dy    uy = ci*dy - si*dx    etx = ux - z.tx    ety = uy - z.ty
 *     a = ci*cj + si*sj    b = ci*sj - si*cj    rc = z.c*a + z.s*b    rs = z.c*b - z.s*a    den = 1.0 + rc    er = (2.0*rs) / den
 * (er is twice the tangent of half the angle of R_z^T R_i^T R_j: no trigonometry anywhere).
 * FLAGS of an edge, decided anew at every linearisation, in this order:
 *     RR_GRAPH_EDGE_BAD      i == j, i >= N or j >= N, a field that is not finite, or a negative weight (no state is read)
 *     RR_GRAPH_EDGE_FLIPPED  den is not >= 2^-20 (the turn is within about a milliradian of pi)
 *     RR_GRAPH_EDGE_BAD      chi below is not finite
 * A flagged edge takes no part in that iteration.  With wt = (double)w_t, wr = (double)w_r:
 *     chi = wt*(etx*etx + ety*ety) + wr*(er*er)        kk = 1.0 + (er*er) / 4.0
 * COST.  chi2 = the sum of chi over the unflagged edges, in the order of REDUCTION below over the edge index (a flagged edge adds 0.0).
 * With robust_k > 0 an edge's weights are scaled once per linearisation: sc = 1.0 / (1.0 + chi / (robust_k*robust_k)), wt = wt*sc,
 * wr = wr*sc (the Cauchy weight of iteratively re-weighted least squares; the record's chi2 stays the unscaled sum).
 * UPDATE.  delta = (dth, dx, dy) per node: t <- t + (dx, dy), R <- R * Cayley(dth), renormalised:
 *     u = dth / 2.0    dc = (1.0 - u*u) / (1.0 + u*u)    ds = (2.0*u) / (1.0 + u*u)
 *     c1 = c*dc - s*ds    s1 = s*dc + c*ds    n = sqrt(c1*c1 + s1*s1)    c = c1/n    s = s1/n    tx = tx + dx    ty = ty + dy
 * A node whose delta is zero in all three components keeps every byte of its state.  The JACOBIANS are the exact derivatives of the
 * residuals under this update (the Cayley turn has unit derivative at 0, and d er / d dth_j = kk):
 *     node i:  d(etx, ety, er) / d(dth, dx, dy) = [ uy -ci -si ; -ux si -ci ; -kk 0 0 ]      node j:  [ 0 ci si ; 0 -si ci ; kk 0 0 ]
 * so a fixed point is a stationary point of the stated cost.
 * GATHER.  Node n adds the terms of its incident unflagged edges IN ASCENDING EDGE INDEX, acc = acc + term from 0.0, by the LIST SUM: a
 * list of at most 64 entries (flagged ones included in the count) is summed one after the other; a longer one is split over 64 lanes, lane
 * l summing entries l, l + 64, l + 128, ... of the list one after the other from 0.0, and the 64 lane sums are then halved:
 * for h = 32, 16, .. 1: lane[t] = lane[t] + lane[t + h] for t < h.  The terms, with nn = ci*ci + si*si:
 *     as node i:  H00 = wt*(uy*uy + ux*ux) + wr*(kk*kk)    H01 = -(wt*(uy*ci + ux*si))    H02 = wt*(ux*ci - uy*si)    H11 = wt*nn
 *                 g0 = wt*(uy*etx - ux*ety) - wr*(kk*er)    g1 = wt*(si*ety - ci*etx)    g2 = -(wt*(si*etx + ci*ety))
 *     as node j:  H00 = wr*(kk*kk)    H01 = 0    H02 = 0    H11 = wt*nn    g0 = wr*(kk*er)    g1 = wt*(ci*etx - si*ety)    g2 = wt*(si*etx + ci*ety)
 * (H22 = H11 and H12 = 0 exactly.)  The node's block is [ H00+lambda H01 H02 ; H01 H11+lambda 0 ; H02 0 H11+lambda ]: lambda is added
 * to the diagonal as it is (H + lambda * I), so a graph without a fixed node needs lambda > 0 for a definite system.  The block is
 * factored by the explicit LDL^T of rr_register_surfels (d0, l10, l20, d1, m21, l21, d2 with H12 = 0); a FIXED node, and a node one of
 * whose pivots is not > 0 (a DEAD block, counted in the record; an unfixed node without edges at lambda = 0), has delta = 0 in this
 * iteration and its rows and columns are dropped.  M^-1 v is that LDL^T's solve (z0 = v0, z1 = v1 - l10*z0, z2 = (v2 - l20*z0) - l21*z1,
 * x2 = z2/d2, x1 = z1/d1 - l21*x2, x0 = (z0/d0 - l10*x1) - l20*x2).
 * SOLVE of (H + lambda*I) delta = -g by preconditioned conjugate gradients, matrix-free, a FIXED count of cg_iterations:
 *     x = 0    r = -g    z = M^-1 r    rz_0 = <r, z>
 *     step k = 0 ..:  p = z (k = 0), else p = z + (rz_k / rz_(k-1)) * p, per component
 *                     q_n = the LIST SUM over n's edges of the product terms below, then q_n = q_n + lambda * p_n per component
 *                     pAp = <p, q>; if pAp or rz_k is not > 0 or not finite: the solve STOPS, the remaining steps of this outer iteration
 *                     are no-ops and k is recorded (decided on the device; -g = 0 stops at k = 0)
 *                     alpha = rz_k / pAp    x = x + alpha*p    r = r - alpha*q    z = M^-1 r    rz_(k+1) = <r, z>
 *     product terms of an edge with pi = p_i, pj = p_j:
 *         v0 = ((uy*pi0 - ci*pi1) - si*pi2) + (ci*pj1 + si*pj2)    v1 = ((si*pi1 - ux*pi0) - ci*pi2) + (ci*pj2 - si*pj1)    v2 = kk*(pj0 - pi0)
 *         y0 = wt*v0    y1 = wt*v1    y2 = wr*v2
 *         as node i:  (uy*y0 - ux*y1) - kk*y2,   si*y1 - ci*y0,   -(si*y0 + ci*y1)        as node j:  kk*y2,   ci*y0 - si*y1,   si*y0 + ci*y1
 * REDUCTION.  <a, b> is ((a0*b0 + a1*b1) + a2*b2) per node (0.0 for a dropped node), then over the node index: values are taken in CHUNKS
 * of 256 consecutive indices (the last one padded with 0.0); inside a chunk for h = 128, 64, .. 1: v[t] = v[t] + v[t + h] for t < h, the
 * chunk's partial is v[0]; the partials P[0 .. m) are combined by s[t] = P[t] + P[t + 256] + P[t + 512] + ... one after the other from 0.0
 * for t = 0..255, and the same halving over s.  chi2 is reduced over the edge index in the same way.
 * An OUTER ITERATION linearises every edge, gathers, solves and updates; `iterations` of them run, then one last linearisation.
 * recs[it], it < iterations: chi2 BEFORE step it, the edges used and flagged, the dead blocks and the step at which the solve stopped
 * (-1: it ran its cg_iterations); recs[iterations]: chi2 and the edge counts of the final states, dead = 0, cg_stop = -1.  Every byte is
 * written.  iterations = 0 returns the states byte for byte and recs[0] with the input's chi2.  edge_flags (one byte per edge, may be
 * NULL) holds the flags of the last linearisation.
 *
 * rr_graph_plan[_device] builds the per-node incidence lists once, on the device without a read-back: a count (integer atomics), a scan,
 * a fill and a per-list sort, so that a node's list is in ascending edge index whichever way it was filled.  The plan depends on the
 * edges' ENDPOINTS and on N and E alone -- an edge with i == j or an index >= N is left out of it; a field that is not finite is found at
 * each linearisation -- and may be reused for any number of solves while the endpoints stay.  Its bytes are a function of the endpoints.
 * rr_optimize_graph_device enqueues on `stream` (NULL: the context's), per outer iteration, a linearisation, a gather, two launches per
 * CG step, an update and a record launch; no host round trip, no workgroup waiting for another (values cross between workgroups at KERNEL
 * BOUNDARIES only), no context memory: all working memory is the caller's d_scratch (rr_graph_scratch_bytes: 96 bytes of terms and a flag
 * byte per edge, 193 bytes per node, and the reductions' partials; its contents before the call do not matter), so solves may run on any
 * streams beside each other and beside batches in flight.  The host forms stage through context-owned buffers and are synchronous.
 * LIMITS: N in 1..2^20, E in 0..2^22 (edges may be NULL iff E == 0), iterations 0..256, cg_iterations 0..1024.
 * Refused with a message and nothing written: -1 for a null ctx; -3 for a null required buffer or config, N or E out of range, iterations
 * or cg_iterations over their caps, a lambda or robust_k that is negative or not finite, a non-zero reserved word, plan_bytes below
 * rr_graph_plan_bytes or scratch_bytes below rr_graph_scratch_bytes, states, edges, records, plan or scratch that are not 16-byte
 * aligned (device forms).  No config of the radar is needed. */
typedef struct rr_graph_edge {   /* 48 B */
    uint32_t i, j;             /* the edge measures node j in node i's frame */
    double c, s, tx, ty;       /* the measured state: a matcher's record with target i and source j */
    float w_t;                 /* 1/m^2: isotropic weight of the translation residual, in i's frame */
    float w_r;                 /* weight of the rotation residual */
} rr_graph_edge;

typedef struct rr_graph_config {   /* 32 B */
    int32_t iterations;        /* 0..256 outer iterations */
    int32_t cg_iterations;     /* 0..1024 CG steps per outer iteration */
    double  lambda;            /* >= 0, added to the diagonal of H */
    double  robust_k;          /* 0: plain least squares; > 0: the Cauchy kernel's scale, in units of sqrt(chi) */
    int32_t reserved_[2];      /* 0 */
} rr_graph_config;

#define RR_GRAPH_EDGE_FLIPPED 1u
#define RR_GRAPH_EDGE_BAD     2u
typedef struct rr_graph_rec {  /* 32 B, every byte written */
    double   chi2;             /* the cost before this record's step (the last record: of the final states) */
    uint32_t n_used;           /* unflagged edges */
    uint32_t n_flipped;        /* edges flagged RR_GRAPH_EDGE_FLIPPED */
    uint32_t n_bad;            /* edges flagged RR_GRAPH_EDGE_BAD */
    uint32_t n_dead;           /* unfixed nodes whose block had a pivot that is not > 0 */
    int32_t  cg_stop;          /* the CG step at which the solve stopped early, or -1 */
    uint32_t reserved_;        /* 0 */
} rr_graph_rec;

/* the blocking of the kernels: nodes per chunk of a reduction, edges per chunk of the linearisation (tests put counts at their edges) */
void   rr_graph_tile_sizes(int* node_chunk, int* edge_tile);
size_t rr_graph_plan_bytes(int n_nodes, int n_edges);                                                 /* 0 for a refused shape */
size_t rr_graph_scratch_bytes(int n_nodes, int n_edges, const rr_graph_config* cfg);                  /* 0 for a refused shape */
int rr_graph_plan_device(rr_ctx* ctx, const rr_graph_edge* d_edges, int n_nodes, int n_edges, void* d_plan, size_t plan_bytes, void* stream);
int rr_graph_plan(rr_ctx* ctx, const rr_graph_edge* edges, int n_nodes, int n_edges, void* plan, size_t plan_bytes);   /* host buffers, synchronous */
int rr_optimize_graph_device(rr_ctx* ctx, double* d_states /*[N][4], in and out*/, const uint8_t* d_fixed /*[N]*/, const rr_graph_edge* d_edges,
                             int n_nodes, int n_edges, const void* d_plan, const rr_graph_config* cfg, rr_graph_rec* d_recs /*[iterations+1]*/,
                             uint8_t* d_edge_flags_or_NULL /*[E]*/, void* d_scratch, size_t scratch_bytes, void* stream);
int rr_optimize_graph(rr_ctx* ctx, double* states, const uint8_t* fixed, const rr_graph_edge* edges, int n_nodes, int n_edges, const void* plan,
                      const rr_graph_config* cfg, rr_graph_rec* recs, uint8_t* edge_flags_or_NULL);   /* host buffers, synchronous */

/* ---- several GPUs of one node behind one object (SURVEY.md §8b "Threading", §8e) -------------------------
 * The reference creates ONE backend object per process (src/radar_simulator.cpp:145-176) and fans out inside it
 * (OpenMP over azimuths, RadarCPU.cpp:155).  rr_multi is that object for n GPUs: one rr_ctx per device, mesh and
 * parameters replicated, device i renders the contiguous azimuth block rr_partition(n_angles, n, i) of every frame
 * of a call in one set of launches, ONE RCCL collective per call over xGMI gathers the blocks on device 0 (one
 * group of send / recv pairs to the root: one piece per device for equal blocks, one per device and frame for ragged
 * ones; no other device receives anything), which transposes them into the mono8 images and copies them to the
 * caller's host buffer.  With one device no collective runs and the images are byte-identical to rr_simulate's.
 * RCCL (librccl.so.1) is loaded at run time when n > 1. */
/* (Test switch RR_MULTI_LOOPBACK=1: a device may be listed several times; the collective is then replaced by
 * device-to-device copies along the same plan -- the n > 1 path on a one-GPU box, minus the RCCL calls.) */
typedef struct rr_multi rr_multi;
rr_multi* rr_create_multi(const int* devices, int n_devices);    /* NULL on failure: rr_multi_last_error(NULL) */
void rr_destroy_multi(rr_multi* m);
const char* rr_multi_last_error(const rr_multi* m);
int rr_multi_device_count(const rr_multi* m);
/* the NCCL version code of the RCCL library this object's communicator was made with (ncclGetVersion: 2.27.7 -> 22707); 0: no
 * communicator (one device, loopback) or a library that does not say.  rr_create_multi refuses a library outside [2.7, 3.0)
 * -- the prototypes it calls through are declared by hand -- and, before the first frame, has every rank send 16 bytes to rank
 * 0 with guard bytes behind them (the constant taken for ncclUint8 must move exactly 16). */
int rr_multi_rccl_version(const rr_multi* m);
rr_ctx* rr_multi_ctx(rr_multi* m, int i);                        /* the context of device i (stats, tuning) */
/* azimuth block [*begin, *end) of `rank` among `world`: contiguous, sizes differ by at most one column */
void rr_partition(int n_angles, int world, int rank, int* begin, int* end);
/* the data plan of one rr_multi_simulate_batch call (pure arithmetic, no GPU): whether the blocks are equal (all-gather
 * of bytes_per_device per device) and, for the ragged case, for device r and frame f (index r * n_frames + f) the byte
 * offset of the piece in r's block buffer, its offset in the root's [n_frames][n_angles][n_cells] buffer and its size */
int rr_multi_plan(int n_angles, int n_cells, int n_devices, int n_frames, int* equal_blocks, size_t* bytes_per_device,
                  size_t* send_off, size_t* recv_off, size_t* piece_bytes);
/* replicated setters: same contracts as the rr_set_* calls above, applied to every device */
/* rr_multi_set_mesh / _gpu: the tree is built ONCE (on the host / on device 0) and copied to the other devices (rr_copy_mesh) */
int rr_multi_set_mesh(rr_multi* m, const float* verts, size_t nv, const uint32_t* faces, size_t nf, const uint32_t* face_object_id);
int rr_multi_set_mesh_gpu(rr_multi* m, const float* verts, size_t nv, const uint32_t* faces, size_t nf, const uint32_t* face_object_id);
/* dynamic scenes: the same contracts on every device; a rebuild runs on device 0 and the tree is copied (rr_copy_mesh) */
int rr_multi_set_object_poses(rr_multi* m, const float* poses, size_t n);
int rr_multi_update_vertices(rr_multi* m, const float* verts, size_t nv);
int rr_multi_rebuild_tree(rr_multi* m, int builder);
int rr_multi_set_materials(rr_multi* m, const rr_material* materials, size_t n_materials,
                           const int32_t* object_materials, size_t n_objects, int32_t material_id_air);
int rr_multi_set_config(rr_multi* m, const rr_config* cfg);
int rr_multi_set_beam_samples(rr_multi* m, const float* dirs, size_t n);
int rr_multi_set_noise_offsets(rr_multi* m, const float* rnd, size_t n);
int rr_multi_set_motion_poses(rr_multi* m, const float* poses, size_t n);
/* Radar::simulate on all devices: one frame / n_frames (1..RR_MAX_BATCH) frames, host output
 * [n_frames][n_cells][n_angles], synchronous; -7 / -8 like rr_simulate when a device reports an overflow / bad id */
int rr_multi_simulate(rr_multi* m, const float pose_qxyzw_t[7], uint8_t* out_u8);
int rr_multi_simulate_batch(rr_multi* m, const float* poses, int n_frames, uint8_t* out_imgs_u8);
/* Pipelined form (what a node that streams frames calls, radar_simulator.cpp:197-212): enqueues the batch and returns;
 * the images are complete only after rr_multi_wait(m, h_imgs_u8) (NULL: every batch in flight), which also reports a
 * -7 / -8 of that batch.  Up to RR_MULTI_SLOTS (default 4, 1..8) batches are in flight -- the render of batch k+1
 * overlaps the collective, the transpose and the D2H copy of batch k; a call that finds its slot still busy waits for
 * that older batch first.  h_imgs_u8 should be page-locked (rr_host_alloc) and handed out from a ring at least as deep
 * as the slots; it must stay valid and unread until waited for.  After any error return nothing of the object is in
 * flight any more (every device drained, error bits cleared): the caller may free its buffers.  AN ERROR INVALIDATES EVERY
 * BATCH IN FLIGHT: error bits are kept per frame lane, not per batch, and the drain reads and clears them all, so the other
 * batches that were in flight report the same code from the rr_multi_wait for their own buffer (or from the call that next
 * uses their slot), whatever their images look like; rr_multi_wait(m, NULL) reports the error once for all of them.
 * With ONE device a batch takes rr_simulate_batch_host_async's route (SDMA, or the stream-ordered copy behind the batch). */
int rr_multi_simulate_batch_async(rr_multi* m, const float* poses, int n_frames, uint8_t* h_imgs_u8);
int rr_multi_wait(rr_multi* m, const void* h_imgs_u8);

/* ---- host side of the seam: what the reference does on the CPU around simulate() (no GPU involved) -----------------
 * Beam samples = sample_cone_local (src/radarays_ros/radar_algorithms.cpp:248-294; erfinvf radar_math.h:13-44):
 * RadarCPU::simulate re-draws m_waves_start whenever a dynamic reconfigure changed beam_width / n_samples /
 * beam_sample_dist / p_in_cone (RadarCPU.cpp:136-145).  rr_cone_dirs is the geometry on caller-supplied variates
 * (u_angle in [0, 1) -> angle, r_variate: U(0,1) for sample_dist 0 / 1, N(0,1) for 2 / 3), bit-equal to the oracle's
 * restatement; rr_sample_cone_local draws the variates itself from a SEEDED MT19937 (the reference seeds from
 * std::random_device: unreproducible) in numpy.random.RandomState's streams, so that it returns the directions
 * radarays_ros_amd/beams.py: sample_cone_local(seed) returns.  width_rad = RadarModel.beam_width (radians);
 * out_dirs [n][3], local azimuth frame, ready for rr_set_beam_samples. */
int rr_cone_dirs(float width_rad, int sample_dist, float p_in_cone, const float* u_angle, const float* r_variate, size_t n,
                 float* out_dirs);
int rr_sample_cone_local(uint32_t seed, float width_rad, size_t n, int sample_dist, float p_in_cone, float* out_dirs);

/* The map file, as rm::import_embree_map(map_file) reads it for the node (src/radar_simulator.cpp:149): PLY (ascii,
 * binary little / big endian; MulRan maps, launch/mulran_sim.launch:7), Wavefront OBJ (objects `o` / `g` become
 * object ids, the index into object_materials) and COLLADA .dae (the reference's default map, launch/mro_husky.launch:4;
 * csrc/rr_collada.cpp: one object per instantiated geometry / primitive group, depth-first in scene order, node
 * transforms and <unit meter> applied, the up axis left as modelled) into the flat arrays rr_set_mesh takes; polygons
 * are fan-triangulated.  The arrays are malloc'ed: give them back with rr_free_mesh.  <0 + text in err on failure. */
typedef struct rr_mesh {
    float* verts;               /* [n_verts][3] */
    size_t n_verts;
    uint32_t* faces;            /* [n_faces][3] */
    size_t n_faces;
    uint32_t* face_object_id;   /* [n_faces] */
    size_t n_objects;           /* OBJ: number of o / g groups, DAE: instantiated primitive groups (>= 1) */
    char** object_names;        /* [n_objects] NUL-terminated names (OBJ group / DAE geometry names), or NULL (PLY):
                                   what to match a scene's material table against */
} rr_mesh;
int rr_load_mesh_file(const char* path, rr_mesh* out, char* err, size_t err_len);
/* Object numbering.  The reference indexes its material table by the object id rmagine's importer hands out
 * (m_object_materials[obj_id], RadarCPU.cpp:268; rm::import_embree_map, radar_simulator.cpp:149; the per-object lists of
 * config/oru4_test.yaml:37-56).  rr_load_mesh_file numbers objects in DEPTH-FIRST SCENE ORDER (OBJ: order of the o / g
 * groups; DAE: instantiated geometries as the visual scene is walked) -- this build's specification; whether rmagine / assimp
 * number a given file the same way cannot be checked without them.  A scene whose material list was written for another
 * numbering is put right here: object `order[k]` becomes id k, objects not listed keep their relative order behind the listed
 * ones; only face_object_id and the order of object_names change.  Unknown, duplicate or ambiguous names are refused. */
int rr_mesh_reorder_objects(rr_mesh* m, const char* const* order, size_t n_order, char* err, size_t err_len);
void rr_free_mesh(rr_mesh* m);

/* ---- environment switches (read at rr_create / at a build; none is needed in normal use) --------------------------
 * RR_LANES (4)            frame buffer sets = batches that can be in flight (1..8)
 * RR_STREAM_LANES (3)     lanes whose own stream rr_simulate_device rotates over
 * RR_STACKLESS (0)        1: k_trace walks the tree WITHOUT a stack (parent links, a node re-fetched each time the walk returns to it;
 *                         no LDS) -- the traversal north_star names, built and measured in round 6: same images, slower
 * RR_HOST_SDMA (1)         rr_simulate_batch_host_async hands a batch's images to the SDMA engines through ROCr (hsa_amd_memory_async_copy,
 *                         a worker thread per context; page-locked destinations) -- the same engine under every HIP runtime; 0: a
 *                         stream-ordered copy behind the batch (the library's copy kernel, or hipMemcpyAsync for a pageable buffer).
 *                         RR_HOST_SDMA_VERBOSE=1 says on stderr why the path was not available or was switched off
 * RR_CULL_POP (1)         later passes drop stack entries at pop time by their distance bound; 0: off (same images)
 * RR_GRAPHS (1)           launch chains of pose batches captured and replayed as hipGraphs (rr_get_graph_stats); 0: kernel by kernel
 * RR_TIGHT_GRID (1)       later-pass trace rows sized by the history of earlier batches (rr_get_trace_grid); 0: the doubling bound
 * RR_TRACE_CHUNK (16)     later-pass trace launches walk chunks of S neighbouring azimuths with the azimuth as the fast grid dimension;
 *                         0: one grid row per azimuth (same images)
 * RR_TIGHT_FORCE (0)      n > 0: rows of n workgroups whatever the history says (tests: nearly every ray goes through the repair launch)
 * RR_STACK_LDS (64)       traversal stack entries kept in LDS (lower: exercises the HBM spill path)
 * RR_PASS0_AZ (16)        neighbouring azimuths per pass-0 wave (1, 2, 4, 8, 16)
 * RR_ROCTX (0)            1: roctx ranges around the kernel enqueues (rocprofv3 --marker-trace)
 * RR_TRACE_STATS          set: rr_get_stats prints the wave-level loop shape of the statistics build
 * RR_BVH_THREADS, RR_BVH_VERBOSE, RR_BVH_ALPHA / _BETA / _BUDGET / _WZ   host builder: threads, phase times, and the
 *                         BvhOptions (csrc/rr_bvh.h) for experiments;  RR_LBVH_NO_SPLIT: GPU builder without split clipping
 * RR_BVH_CHOOSE (1)       host builder, meshes up to 2M triangles: build the candidates (SAH with spatial splits; plain SAH with
 *                         vertical weight 0.5 / 1.0), trace one sample of radar-like rays through each, keep the tree with
 *                         the fewest traversal steps; 0: the default tree only (images are the same whichever tree)
 * RR_METRICS_HIST (0)     1: rr_compare_images_device counts its joint histograms with global atomics instead of workgroup-private
 *                         LDS histograms (the same counts, measured 24-32x slower: BASELINE.md §10; kept selectable for
 *                         tools/probe_metrics.py)
 * RR_MULTI_LOOPBACK (0)   1: rr_create_multi accepts one device several times (tests, see above)
 * RR_MULTI_SELF_RCCL (0)  1 with ONE device: its block travels to itself through the real RCCL calls (one-rank communicator, a
 *                         group of ncclSend / ncclRecv to self; 2: one pair per frame, the ragged plan) instead of the
 *                         single-device route (tests on one-GPU boxes)
 * RR_MULTI_THREADS (0)    1: rr_multi with several devices starts one enqueue thread per device, which issues that device's
 *                         launches of a call while the others issue theirs (off by default: on one physical device, the
 *                         only case measurable on a one-GPU box, the runtime serialises the threads and nothing is gained)
 * RR_MULTI_SLOTS (4)      batches rr_multi keeps in flight (streams + buffer sets per device, 1..8)
 * RR_HOST_PROFILE (0)     1: where the HOST time of the batch calls goes (named scopes in rr_ctx / rr_multi, csrc/rr_hostprof.h);
 *                         a table on stderr when the process ends (read it with RR_MULTI_THREADS=0) */

#ifdef __cplusplus
}
#endif
#endif
