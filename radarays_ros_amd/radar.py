"""Host-side mirror of the reference's backend interface for this path.

Reference seam (C++):   class Radar { virtual sensor_msgs::ImagePtr simulate(ros::Time) = 0; }
                        include/radarays_ros/Radar.hpp:34-105, src/radarays_ros/Radar.cpp
Backends there:         RadarCPU (Embree), RadarGPU (OptiX) -- chosen in radar_simulator.cpp:118-176.
`RadarHIP` is the third backend: same member names / same argument meaning /
same error behaviour (simulate() returns None when no transform is known, like
the null ImagePtr of RadarCPU.cpp:129-133), on top of libradarays_mi355.so.
ROS itself is absent here: TF lookup is replaced by updateTsm(pose) and the
returned message is a plain `Image` object with sensor_msgs/Image's fields.
"""
from dataclasses import dataclass, field

import numpy as np

from . import beams, native, scenes
from .params import (N_ANGLES, WAVE_ENERGY_THRESHOLD, RadarModelConfig, RadarParams,
                     default_params)


unpack_info = native.unpack_info      # info word of an echo / label pixel -> (object, pass, kind)


# ---- wave paths: pure-numpy helpers over the records of simulate_paths (native.WAVE_DTYPE, ONE azimuth's list unless said otherwise)
def unpack_wave_info(info):
    """the info word of a wave record -> (object id, pass, branch, has_path_echo, has_multipath_echo); a miss has object 0xFFFFFF;
    branch 0: emitted beam, 1: reflection child, 2: transmission child.  Arrays or scalars."""
    i = np.asarray(info, np.uint32)
    return (i & np.uint32(0xFFFFFF), (i >> np.uint32(24)) & np.uint32(15), (i >> np.uint32(28)) & np.uint32(3),
            (i >> np.uint32(30)) & np.uint32(1), (i >> np.uint32(31)) & np.uint32(1))


def hit_points(records):
    """o + range * d of every record (f32, any shape of records -> [..., 3]); NaN for a wave that missed."""
    r = np.asarray(records)
    rng = r["range"].astype(np.float32)
    p = r["o"] + rng[..., None] * r["d"]
    p[rng < 0] = np.nan
    return p.astype(np.float32)


def path_to_wave(records, i):
    """the chain of waves from the emitted beam to wave i of one azimuth's list: their indices, beam first (walks `parent`)."""
    r = np.asarray(records)
    chain = []
    i = int(i)
    while i >= 0:
        if i >= len(r):
            raise IndexError("wave %d lies beyond the %d records given (a truncated list?)" % (i, len(r)))
        if len(chain) > 16:
            raise ValueError("parent chain longer than the pass limit: not a wave list")
        chain.append(i)
        i = int(r["parent"][i])
    return np.array(chain[::-1], np.int64)


def path_to_echo(records, k):
    """a ghost's route: the wave that owns echo k of the azimuth's echo stream, traced back to the beam ->
    (wave indices beam first, polyline f32 [len + 1][3]: the beam's start point, then the hit point of every wave of the chain)."""
    r = np.asarray(records)
    k = int(k)
    _, _, _, e0, e1 = unpack_wave_info(r["info"])
    n_own = e0.astype(np.int64) + e1.astype(np.int64)
    own = np.nonzero((r["echo"] >= 0) & (r["echo"] <= k) & (k < r["echo"] + n_own))[0]
    if len(own) != 1:
        raise IndexError("echo %d is owned by %d of the %d records given" % (k, len(own), len(r)))
    chain = path_to_wave(r, own[0])
    pts = np.concatenate([r["o"][chain[:1]], hit_points(r[chain])]).astype(np.float32)
    return chain, pts


@dataclass
class Header:
    stamp: float = 0.0
    frame_id: str = ""


@dataclass
class Image:
    """sensor_msgs/Image as RadarCPU.cpp:555-561 fills it."""
    header: Header = field(default_factory=Header)
    height: int = 0
    width: int = 0
    encoding: str = "mono8"
    is_bigendian: int = 0
    step: int = 0
    data: np.ndarray = None     # [height][width] uint8


class RadarHIP:
    def __init__(self, verts, faces, face_object_id=None, map_frame="map", sensor_frame="sensor",
                 device=0, beam_seed=42):
        self.m_map_frame = map_frame
        self.m_sensor_frame = sensor_frame
        self.m_params: RadarParams = default_params()          # Radar.cpp:22
        self.m_material_id_air = 0                             # Radar.cpp:23
        self.m_wave_energy_threshold = WAVE_ENERGY_THRESHOLD   # Radar.cpp:24
        self.m_resample = True                                 # Radar.cpp:25
        self.m_object_materials = []
        self.m_cfg = RadarModelConfig()
        self.m_waves_start = None
        self.Tsm_last = None
        self._beam_seed = beam_seed
        self._noise_seed = 7
        self._motion = None
        self._ctx = native.Context(device)
        self._ctx.set_mesh(verts, faces, face_object_id)
        self._dirty_cfg = True
        self._dirty_mat = True
        self.updateDynCfg(self.m_cfg)

    # -- Radar.cpp:220-226
    def loadParams(self, materials, object_materials, material_id_air=0):
        self.m_params.materials = list(materials)
        self.m_object_materials = list(object_materials)
        self.m_material_id_air = int(material_id_air)
        self._dirty_mat = True

    def getParams(self):
        return self.m_params

    def setParams(self, params: RadarParams):
        self.m_params = params
        self._dirty_mat = True
        self._dirty_cfg = True

    # -- Radar.cpp:188-218
    def updateDynCfg(self, config: RadarModelConfig, level=0):
        old = self.m_cfg
        if (config.beam_sample_dist != old.beam_sample_dist
                or abs(config.beam_width - old.beam_width) > 0.001
                or config.n_samples != old.n_samples
                or abs(config.beam_sample_dist_normal_p_in_cone - old.beam_sample_dist_normal_p_in_cone) > 0.001):
            self.m_resample = True
        self.m_params.model.beam_width = config.beam_width * np.pi / 180.0
        self.m_params.model.n_samples = config.n_samples
        self.m_params.model.n_reflections = config.n_reflections
        self.m_cfg = config.copy()
        self._dirty_cfg = True

    # -- Radar.cpp:80-132 (TF lookup replaced by an explicit pose)
    def updateTsm(self, pose_qxyzw_t=None):
        if pose_qxyzw_t is not None:
            p = np.asarray(pose_qxyzw_t, np.float32)
            if p.shape != (7,) or not np.all(np.isfinite(p)):
                return False
            self.Tsm_last = p
        return self.Tsm_last is not None

    def setBeamSamples(self, dirs):
        """Inject m_waves_start (tests use the committed fixture)."""
        self.m_waves_start = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        self.m_resample = False
        self._ctx.set_beam_samples(self.m_waves_start)

    def setMotionPoses(self, poses):
        """include_motion (cfg/RadarModel.cfg:85): the pose TF would return at each azimuth
        (RadarCPU.cpp:190-196), [400][7]; None -> one pose per frame."""
        self._motion = None if poses is None else np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        self._ctx.set_motion_poses(self._motion)
        if self._motion is not None:
            self.Tsm_last = self._motion[-1].copy()

    def setNoiseOffsets(self, rnd):
        self._ctx.set_noise_offsets(rnd)

    # ---- dynamic scenes: one rigid pose per object of face_object_id, the tree refit in place (include/radarays_mi355.h)
    def setObjectPoses(self, poses):
        """[n_objects][7] = qx qy qz qw tx ty tz: frames simulated after this call see every object moved by its pose."""
        self._ctx.set_object_poses(poses)

    def updateVertices(self, verts):
        """new rest vertices (same count and faces as the loaded mesh); the object poses stay."""
        self._ctx.update_vertices(verts)

    def rebuildTree(self, builder="host"):
        """a fresh tree of the posed scene ("host" or "gpu" builder): worth it when treeCost() has grown."""
        self._ctx.rebuild_tree(builder)

    def treeCost(self):
        """(cost of the current boxes, cost of the tree as built)."""
        return self._ctx.tree_cost()

    # ---- point clouds and Cartesian images of polar images, on the GPU (rr_detect.hip; the reference runs
    # radar_tools/radar_img_to_pcl on every image, launch/tests/radar_sim_test.launch:80-84).  cfg: rr_detect_config fields
    # (method 0 / "cfar", 1 / "kstrongest"; native.DETECT_DEFAULTS for the rest)
    def _polar(self, image):
        return image.data if isinstance(image, Image) else np.asarray(image)

    def toPointCloud(self, image, **cfg):
        """one mono8 polar Image (simulated or real, this model's shape) -> POINT_DTYPE array: x, y, z in the sensor frame of
        each point's azimuth, intensity, column, bin; sorted by column, then bin"""
        self._push()
        pts, _ = self._ctx.detect(self._polar(image), cfg)
        return pts[0]

    def toCartesian(self, image, width, pixel_size, bilinear=True, stamp=0.0):
        """one mono8 polar Image -> a mono8 width x width bird's-eye Image (forward = up, left = left, pixel_size m/pixel)"""
        self._push()
        u8 = self._ctx.polar_to_cartesian(self._polar(image), width, pixel_size, bilinear)[0]
        return Image(header=Header(stamp=stamp, frame_id=self.m_sensor_frame), height=u8.shape[0], width=u8.shape[1],
                     encoding="mono8", step=u8.shape[1], data=u8)

    def detectWindow(self, image, mask=False, **cfg):
        """one mono8 polar Image -> POINT_DTYPE array as toPointCloud, by the windowed CFAR (rr_window.hip; cfg: rr_window_detect_config
        fields, method 0 / "ca", 1 / "go", 2 / "so", 3 / "os", native.WINDOW_DEFAULTS for the rest); with mask=True also the uint8
        detection mask [n_cells][n_angles], 255 at a detection"""
        self._push()
        out = self._ctx.detect_window(self._polar(image), cfg, mask=mask)
        return (out[0][0], out[2][0]) if mask else out[0][0]

    def simulatePointClouds(self, poses, window=None, **cfg):
        """[n][7] poses -> n point clouds (POINT_DTYPE arrays).  Per 64 poses: rr_simulate_batch_device and rr_detect_device on
        one stream into device buffers; only the offsets and the points come to the host, no image does.  window (a dict of
        rr_window_detect_config fields or a native.window_detect_config; {}: its defaults): rr_detect_window_device detects instead"""
        import torch
        self._push()
        if window is None:
            det = native.detect_config(cfg, n_cells=self.m_cfg.n_cells)
        elif cfg:
            raise ValueError("window= comes without rr_detect_config fields, got %s" % sorted(cfg))
        else:
            det = native.window_detect_config(window, n_cells=self.m_cfg.n_cells, n_angles=N_ANGLES)
        poses = native.object_poses_array(poses)
        dev = torch.device("cuda", self._ctx.device)
        out = []
        # an explicit stream: the library reads a null handle as "the context's own stream", torch as its default stream
        stream = torch.cuda.Stream(device=dev)
        s = stream.cuda_stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            for _, n, _, pts, _, totals in self._detected_chunks(poses, det, s, capped=False):
                host = pts.cpu().numpy().view(native.POINT_DTYPE)
                out.extend(host[f, :int(totals[f])].copy() for f in range(n))
        self._ctx.synchronize(s)
        return out

    def _detected_chunks(self, poses, det, s, capped):
        """The per-64-poses device loop under simulatePointClouds, registerPointClouds and buildLikelihoodField.  Per chunk:
        rr_simulate_batch_device and rr_detect_device on the stream `s` into fresh device tensors -> (offset of the chunk, n, offs int32
        [n][401], pts uint8 [n][max_points * 24], max_points, the counted totals uint32 [n] or None).  capped False: room for every
        detection, which a count-only call finds first.  capped True: k * 400 with k-strongest and no count-only call, what that call
        finds with CA-CFAR, ICP_MAX_POINTS at the most.
        The caller holds the `with` of the stream and iterates inside it: what it allocates before the loop and copies home after it
        belongs on that stream too, and a generator suspended inside a `with` of its own would keep torch on the stream for as long as
        an error raised in the caller's loop body is held."""
        import torch
        n_cells = self.m_cfg.n_cells
        dev = torch.device("cuda", self._ctx.device)
        windowed = isinstance(det, native.RRWindowDetectConfig)          # (simulatePointClouds alone passes one, uncapped)

        def detect(d_imgs, n, d_pts, mp, d_offs):
            if windowed:
                self._ctx.detect_window_device(d_imgs, n, det, d_pts, mp, d_offs, None, s)
            else:
                self._ctx.detect_device(d_imgs, n, det, d_pts, mp, d_offs, s)
        for at in range(0, len(poses), 64):
            chunk = poses[at:at + 64]
            n = len(chunk)
            imgs = torch.empty((n, n_cells, N_ANGLES), dtype=torch.uint8, device=dev)
            offs = torch.empty((n, N_ANGLES + 1), dtype=torch.int32, device=dev)
            self._ctx.simulate_batch_device(chunk, imgs.data_ptr(), s)
            if capped and not windowed and det.method == 1:
                totals, mp = None, det.k * N_ANGLES
            else:
                detect(imgs.data_ptr(), n, None, 0, offs.data_ptr())     # counts
                totals = offs[:, -1].cpu().numpy().view(np.uint32)
                mp = int(totals.max())
            if capped:
                mp = min(mp, native.ICP_MAX_POINTS)
            mp = max(1, mp)
            pts = torch.empty((n, mp * native.POINT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            detect(imgs.data_ptr(), n, pts.data_ptr(), mp, offs.data_ptr())
            yield at, n, offs, pts, mp, totals

    # ---- sweep compensation (rr_deskew.hip): a sweep under motion, as the sensor records it and with the distortion taken out again
    def simulate_sweep(self, pose_ref, twist, sweep_time, gain=0.0, detect=None, cartesian=None, ref_azimuth=0):
        """One sweep of a sensor that moves with the constant body twist `twist` (vx vy vz wx wy wz, sensor frame) for `sweep_time` seconds;
        pose_ref [7] is its pose when azimuth `ref_azimuth` is measured.  scenes.sweep_poses makes the per-azimuth poses; they are installed
        as the motion table, the frame is simulated (through the Doppler call with the sensor's velocity when gain != 0, the plain call
        otherwise), detected and compensated into the frame of pose_ref.  detect: a dict of rr_detect_config fields ({}: the defaults) or
        None for no points; cartesian: a dict(width=, pixel_size=, bilinear=True, iterations=2) or None for no bird's-eye images.
        Returns a dict: image (u8 [n_cells][400], distorted), poses [400][7], sensor_vel [3], table (native.SWEEP_DTYPE [400]), and, as asked
        for, points_raw / offsets / points and cartesian_raw / cartesian.  The context's motion table is left as it was found, also when
        a call raises."""
        poses, vel = scenes.sweep_poses(pose_ref, twist, sweep_time, N_ANGLES, ref_azimuth)
        ref = np.ascontiguousarray(pose_ref, np.float32)
        gain = float(gain)
        self._push()
        ctx = self._ctx
        out = {"poses": poses, "sensor_vel": vel}
        ctx.set_motion_poses(poses)
        try:
            if gain != 0.0:
                out["image"] = ctx.simulate_doppler(ref, sensor_vel=vel, gain=gain, echo_stride=0, want_vel_img=False)[0]
            else:
                out["image"] = ctx.simulate(ref)[0]
            table = ctx.sweep_table(poses, ref, vel if gain != 0.0 else None, gain)
            out["table"] = table[0]
            if detect is not None:
                pts, offs = ctx.detect(out["image"], detect)
                out["points_raw"], out["offsets"] = pts[0], offs[0]
                out["points"] = ctx.compensate_points(pts, offs, table)[0]
            if cartesian is not None:
                c = dict(cartesian)
                width, ps, bil, it = c.pop("width"), c.pop("pixel_size"), c.pop("bilinear", True), c.pop("iterations", 2)
                if c:
                    raise ValueError("unknown cartesian fields: %s" % sorted(c))
                out["cartesian_raw"] = ctx.polar_to_cartesian(out["image"], width, ps, bil)[0]
                out["cartesian"] = ctx.polar_to_cartesian_sweep(out["image"], table, width, ps, bil, it)[0]
        finally:
            ctx.set_motion_poses(self._motion)
        return out

    # ---- object annotations (rr_notes.hip): one record per object and frame, the labels never leave the GPU
    def simulate_annotations(self, poses, extent=native.NOTE_DIRECT, want_images=False):
        """[n][7] poses -> (native.NOTE_DTYPE [n][n_objects], skipped uint32 [n], images or None): per 64 poses one provenance chain
        and its annotation (rr_simulate_batch_annotations).  `extent`: the pixel classes that feed the extents, a mask of
        native.NOTE_DIRECT | NOTE_GHOST | NOTE_MULTIPATH or class names."""
        self._push()
        poses = native.object_poses_array(poses)
        mask = native.note_mask(extent)
        notes, skipped, imgs = [], [], []
        for at in range(0, len(poses), 64):
            n, k, im = self._ctx.simulate_batch_annotations(poses[at:at + 64], mask, want_images)
            notes.append(n); skipped.append(k); imgs.append(im)
        return np.concatenate(notes), np.concatenate(skipped), (np.concatenate(imgs) if want_images else None)

    # ---- the "real to sim gap" (launch/tests/eval_real_to_sim.launch) and the optimiser's other objectives
    # (scripts/radaray_opti.py imports SSIM, PSNR, NMI, VoI and mutual information), on the GPU (rr_metrics.hip)
    def compareImages(self, images, real, which=native.METRIC_ALL, win_size=7):
        """mono8 polar Images (or arrays; one or a list, this model's shape) against ONE real image -> a native.METRICS_DTYPE
        array with one record per image: psnr, sse, ssim, hx, hy, hxy, mi, nmi, voi (fields not asked for are 0)"""
        self._push()
        if isinstance(images, Image) or (isinstance(images, np.ndarray) and images.ndim == 2):
            images = [images]
        return self._ctx.compare_images(np.stack([self._polar(im) for im in images]), self._polar(real), which, win_size)

    # ---- azimuth registration (rr_align.hip): a real sweep and a simulated one do not start at the same azimuth
    def alignImages(self, images, real, cell_begin=0, cell_end=None, want_curve=False):
        """mono8 polar Images (or arrays; one or a list, this model's shape) against ONE real image -> a native.ALIGN_DTYPE array
        with one record per image: the circular azimuth shift (the amount to add to scroll_image) at which the image matches
        `real` best over the cell window [cell_begin, cell_end), and xcorr, sse, psnr, ncc there; with want_curve also xcorr at
        every shift, int64 [n][n_angles]"""
        self._push()
        if isinstance(images, Image) or (isinstance(images, np.ndarray) and images.ndim == 2):
            images = [images]
        return self._ctx.align_images(np.stack([self._polar(im) for im in images]), self._polar(real), cell_begin, cell_end, want_curve)

    # ---- translation registration (rr_shift.hip): x and y of a planar pose from the Cartesian images
    def registerTranslation(self, images, real, width, pixel_size, max_shift, bilinear=True):
        """mono8 polar Images (or arrays; one or a list, this model's shape) and ONE real image, all made Cartesian (width x width,
        pixel_size m/pixel) and compared over -max_shift..max_shift pixels -> (a native.SHIFT_DTYPE array with one record per
        image: (dy, dx) where the image's content is found in `real`, and xcorr, sse, psnr, ncc there; the correction to add to
        each image's pose in the sensor's own axes, metres [n][2] = (forward, left) = (dy + sub_dy, dx + sub_dx) * pixel_size)"""
        self._push()
        if isinstance(images, Image) or (isinstance(images, np.ndarray) and images.ndim == 2):
            images = [images]
        polar = np.stack([self._polar(im) for im in images] + [self._polar(real)])       # the real image rides behind: one conversion
        cart = self._ctx.polar_to_cartesian(polar, width, pixel_size, bilinear)
        rec = self._ctx.shift_images(cart[:-1], cart[-1], max_shift)
        return rec, self._translation(rec, pixel_size)

    @staticmethod
    def _translation(rec, pixel_size):
        return np.stack([(rec["dy"] + rec["sub_dy"]) * pixel_size, (rec["dx"] + rec["sub_dx"]) * pixel_size], axis=1)

    def registerPose(self, poses, real, width, pixel_size, max_shift, bilinear=True, cell_begin=0, cell_end=None):
        """[n][7] simulated poses (qx qy qz qw tx ty tz) of a planar sensor against ONE real polar image -> (corrected poses
        float32 [n][7], the native.ALIGN_DTYPE records of the yaw step, the native.SHIFT_DTYPE records of the translation step).
        Per 64 poses: simulate_batch_align gives each pose's azimuth shift s, a turn of -s * theta_inc about the sensor's z axis;
        the turned poses are simulated again and simulate_batch_shift gives their translation in the sensor's own axes."""
        self._push()
        p = np.array(poses, np.float32).reshape(-1, 7)
        real = self._polar(real)
        theta_inc = float(self._ctx._rrcfg.theta_inc)
        out, yaw_recs, shift_recs = [], [], []
        for at in range(0, len(p), 64):
            chunk = p[at:at + 64].astype(np.float64)
            _, yaw, _ = self._ctx.simulate_batch_align(chunk, real, cell_begin, cell_end)
            s = yaw["shift"].astype(np.int64)
            s = np.where(2 * s > N_ANGLES, s - N_ANGLES, s)           # x was rendered s azimuth steps ahead of `real`
            half = -0.5 * s * theta_inc
            bz, bw = np.sin(half), np.cos(half)                       # q * (0, 0, bz, bw): a turn in the sensor's own frame
            ax, ay, az, aw = chunk[:, 0].copy(), chunk[:, 1].copy(), chunk[:, 2].copy(), chunk[:, 3].copy()
            chunk[:, 0], chunk[:, 1] = ax * bw + ay * bz, ay * bw - ax * bz
            chunk[:, 2], chunk[:, 3] = aw * bz + az * bw, aw * bw - az * bz
            _, sh, _ = self._ctx.simulate_batch_shift(chunk, real, width, pixel_size, max_shift, bilinear)
            v = np.concatenate([self._translation(sh, pixel_size), np.zeros((len(chunk), 1))], axis=1)
            u, w = chunk[:, :3], chunk[:, 3:4]
            uv = np.cross(u, v)
            chunk[:, 4:7] += v + 2.0 * (w * uv + np.cross(u, uv))     # the correction turned into the map frame
            out.append(chunk.astype(np.float32)); yaw_recs.append(yaw); shift_recs.append(sh)
        return np.concatenate(out), np.concatenate(yaw_recs), np.concatenate(shift_recs)

    # ---- scan matching (rr_icp.hip): the planar pose from point clouds, both angles and both translations in one step
    def registerPointClouds(self, poses, real_points, detect=None, gate=1.0, iterations=10, compensate=None):
        """[n][7] pose hypotheses (qx qy qz qw tx ty tz) of a planar sensor against ONE real point cloud (POINT_DTYPE, e.g. toPointCloud
        of a real scan, at most 65,536 points) -> (native.ICP_DTYPE records [n], corrected poses float32 [n][7]).
        Per 64 poses: rr_simulate_batch_device, rr_detect_device (detect: a dict of rr_detect_config fields, None: the defaults; room for
        k * 400 points with k-strongest, for what a count-only pass finds with CA-CFAR, 65,536 at most) and rr_register_points_device on
        one stream from the identity guess; compensate: a native.SWEEP_DTYPE table [400] that rr_compensate_points_device applies to every
        simulated cloud first, or None.  Only the records come to the host.
        Convention: the source is the cloud simulated at the hypothesis X_h, the target the real cloud taken at the true pose X, both in
        their sensor's frame.  A record's (c, s, tx, ty) is T with q ~ T p, so T = X^-1 X_h and the corrected pose is X_h T^-1: the
        hypothesis turned by -atan2(s, c) about its own z axis and moved by -R^T t in its own axes (forward, left)."""
        import torch  # noqa: F401  (a missing torch is reported before any argument, as it always was)
        self._push()
        det = native.detect_config(detect, n_cells=self.m_cfg.n_cells)
        p = native.object_poses_array(poses)
        tgt = native._scan(np.ascontiguousarray(real_points), 1, "real_points")      # ascontiguousarray: one record alone is a cloud of one
        it, g = native._int_in(iterations, 0, 64, "iterations"), native._icp_gate(gate)
        table = None if compensate is None else self._ctx._sweep_records(compensate, 1)
        rec = self._register_chunks(p, det, tgt, len(tgt), self._ctx.register_points_device, g, it, table)
        return rec, self._corrected_by(p, rec)

    def _register_chunks(self, p, det, tgt, count, register_device, g, it, table=None):
        """the loop under both matchers: the target records uploaded once with their count, then per chunk of hypotheses simulate, detect,
        the sweep table (or None) applied to the simulated clouds, and `register_device` from the identity guess, on one explicit stream
        (as simulatePointClouds) -> the records of all chunks.  Only the records come to the host."""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
        recs = []
        stream = torch.cuda.Stream(device=dev)
        s = stream.cuda_stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            d_tgt, d_cnt = up(tgt), up(np.array([count], np.uint32))
            for _, n, offs, pts, mp, _ in self._detected_chunks(p, det, s, capped=True):
                d_rec = torch.empty(n * native.ICP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                if table is not None:
                    d_tab = up(np.tile(table, (n, 1)))
                    self._ctx.compensate_points_device(pts.data_ptr(), offs.data_ptr(), n, mp, d_tab.data_ptr(), None, s)
                register_device(pts.data_ptr(), offs.data_ptr(), n, mp, d_tgt.data_ptr(), d_cnt.data_ptr(), count, d_rec.data_ptr(), None, g, it, None, s)
                recs.append(d_rec.cpu().numpy().view(native.ICP_DTYPE).copy())
        self._ctx.synchronize(s)
        return np.concatenate(recs) if recs else np.zeros(0, native.ICP_DTYPE)

    # ---- oriented surface points and point-to-line scan matching (rr_surfels.hip)
    def surfacePoints(self, points, surfel_cfg, max_surfels=4096):
        """ONE point cloud (POINT_DTYPE, e.g. toPointCloud of a scan, at most 65,536 points) or a list of them -> (a list with one
        native.SURFEL_DTYPE array per cloud: its oriented surface points in ascending cell order, counts uint32 [n][2] = (kept, flags))
        by rr_surface_points.  surfel_cfg: native.surfel_config or a dict of its arguments."""
        self._push()
        pts = native._cloud_list(points)
        offs = np.zeros((len(pts), N_ANGLES + 1), np.uint32)
        offs[:, -1] = [len(p) for p in pts]                           # (the calls read a frame's total only)
        return self._ctx.surface_points(pts, offs, surfel_cfg, max_surfels)

    def registerSurfacePoints(self, poses, real_points, surfel_cfg, detect=None, gate=1.0, iterations=10, max_surfels=4096):
        """registerPointClouds with a point-to-line residual: the real cloud is reduced to oriented surface points once (surfacePoints), and
        per 64 poses rr_simulate_batch_device, rr_detect_device and rr_register_surfels_device run on one stream from the identity guess.
        -> (native.ICP_DTYPE records [n], corrected poses float32 [n][7]).  The pose convention is registerPointClouds': T = X^-1 X_h and
        the corrected pose is X_h T^-1."""
        import torch  # noqa: F401
        self._push()
        det = native.detect_config(detect, n_cells=self.m_cfg.n_cells)
        p = native.object_poses_array(poses)
        it, g = native._int_in(iterations, 0, 64, "iterations"), native._icp_gate(gate)
        tgt = self.surfacePoints(native._scan(np.ascontiguousarray(real_points), 1, "real_points"), surfel_cfg, max_surfels)[0][0]
        if len(tgt) > native.ICP_MAX_POINTS:
            raise ValueError("the target may hold at most %d surface points" % native.ICP_MAX_POINTS)
        rec = self._register_chunks(p, det, tgt if len(tgt) else np.zeros(1, native.SURFEL_DTYPE), len(tgt), self._ctx.register_surfels_device, g, it)
        return rec, self._corrected_by(p, rec)

    # ---- pose-graph optimisation (rr_graph.hip)
    def optimizePoseGraph(self, states, fixed, edges, iterations=10, cg_iterations=50, lam=0.0, robust_k=0.0, plan=None):
        """The back end behind the matchers: float64 states [N][4] = (c, s, tx, ty) (native.se2_states; e.g. the integrated odometry), a
        fixed flag per node and native.GRAPH_EDGE_DTYPE edges (native.graph_edges packs matcher records: edge k says that node j sits at the
        record's state in node i's frame) -> (the optimised states, native.GRAPH_REC_DTYPE [iterations + 1]: chi2 before every step and of
        the result, the edges used and flagged, the dead blocks, the CG step at which a solve stopped) by rr_optimize_graph.  robust_k > 0
        turns the Cauchy kernel on against false closures; lam is added to the diagonal (a graph without a fixed node needs lam > 0);
        plan: Context.graph_plan of these endpoints, to reuse it across solves.  The states go on to buildOccupancyMap as they are."""
        return self._ctx.optimize_graph(states, fixed, edges, native.graph_config(iterations, cg_iterations, lam, robust_k), plan=plan)

    @staticmethod
    def _corrected_by(poses, rec):
        """X_h T^-1 for every hypothesis and its record (registerPointClouds says why)"""
        out = poses.astype(np.float64)
        c, s, tx, ty = rec["c"], rec["s"], rec["tx"], rec["ty"]
        v = np.stack([-(c * tx + s * ty), -(-s * tx + c * ty), np.zeros(len(rec))], axis=1)      # -R^T t, in the hypothesis' own axes
        u, w = out[:, :3].copy(), out[:, 3:4].copy()
        uv = np.cross(u, v)
        out[:, 4:7] += v + 2.0 * (w * uv + np.cross(u, uv))           # ... turned into the map frame
        half = -0.5 * np.arctan2(s, c)
        bz, bw = np.sin(half), np.cos(half)                           # q * (0, 0, bz, bw): a turn in the sensor's own frame
        ax, ay, az, aw = u[:, 0], u[:, 1], u[:, 2], w[:, 0]
        out[:, 0], out[:, 1] = ax * bw + ay * bz, ay * bw - ax * bz
        out[:, 2], out[:, 3] = aw * bz + az * bw, aw * bw - az * bz
        return out.astype(np.float32)

    # ---- likelihood field (rr_field.hip): a map of keyframe clouds as a distance field, and very many pose hypotheses scored against it
    @staticmethod
    def _planar_states(poses):
        """[n][7] poses -> float64 [n][4] = (cos yaw, sin yaw, x, y): the planar part of a pose, sensor frame into the map frame"""
        p = np.asarray(poses, np.float64)
        qx, qy, qz, qw = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
        yaw = np.arctan2(2.0 * (qw * qz + qx * qy), 1.0 - 2.0 * (qy * qy + qz * qz))
        return native.se2_states(yaw, p[:, 4], p[:, 5])

    def buildLikelihoodField(self, poses, field_cfg, detect_cfg=None):
        """[n][7] keyframe poses of a planar sensor -> the likelihood field uint16 [height][width] of the map their scans make
        (field_cfg: native.field_config).  Per 64 poses: rr_simulate_batch_device, rr_detect_device (detect_cfg: a dict of rr_detect_config
        fields, None: the defaults) and rr_rasterize_points_device, every cloud under the planar part of its own pose, into one occupancy
        grid on one stream; then rr_distance_field_device.  Nothing but the field leaves the GPU.
        Convention: a state (c, s, tx, ty) maps a cloud's sensor frame into the map frame, q = R p + t; a keyframe's state is the planar
        part of its pose, (cos yaw, sin yaw, x, y)."""
        import torch
        self._push()
        det = native.detect_config(detect_cfg, n_cells=self.m_cfg.n_cells)
        g = native._field_cfg(field_cfg)
        p = native.object_poses_array(poses)
        if len(p) == 0:
            raise ValueError("a map needs at least one pose")
        states = self._planar_states(p)
        dev = torch.device("cuda", self._ctx.device)
        stream = torch.cuda.Stream(device=dev)      # an explicit stream, as simulatePointClouds
        s = stream.cuda_stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            occ = torch.zeros((g.height, g.width), dtype=torch.uint8, device=dev)
            field = torch.empty((g.height, g.width), dtype=torch.int16, device=dev)
            for at, n, offs, pts, mp, _ in self._detected_chunks(p, det, s, capped=True):
                d_st = torch.from_numpy(np.ascontiguousarray(states[at:at + 64])).to(dev)
                self._ctx.rasterize_points_device(pts.data_ptr(), offs.data_ptr(), n, mp, g, occ.data_ptr(), d_st.data_ptr(), s)
            self._ctx.distance_field_device(occ.data_ptr(), g, field.data_ptr(), 1, s)
            out = field.cpu().numpy().view(np.uint16).copy()
        self._ctx.synchronize(s)
        return out

    def scorePoses(self, scan_points_or_image, states, field, field_cfg, detect_cfg=None):
        """One observed scan against float32 states [n][4] (native.pose_lattice makes them) and a field of buildLikelihoodField ->
        native.FIELD_DTYPE [n] (sum_d2, n_in, n_hit); lower sum_d2 is better.  The scan is a POINT_DTYPE cloud (e.g. toPointCloud of a
        real scan) or a mono8 polar image [n_cells][400], which is detected first (detect_cfg as in buildLikelihoodField).
        Convention: a hypothesis state (c, s, tx, ty) maps the scan's sensor frame into the map frame."""
        self._push()
        scan, _ = self._scan_or_image(scan_points_or_image, detect_cfg)
        return self._ctx.score_poses(scan, states, field, field_cfg)

    def _scan_or_image(self, scan_points_or_image, detect_cfg):
        """a POINT_DTYPE cloud, or a mono8 polar image, which is detected first -> (the cloud, the offsets uint32 [1][401] of the detection
        or None for a cloud that was given)"""
        scan = np.asarray(scan_points_or_image)
        if scan.dtype == native.POINT_DTYPE:
            return scan, None
        pts, offs = self._ctx.detect(self._polar(scan_points_or_image), native.detect_config(detect_cfg, n_cells=self.m_cfg.n_cells))
        return pts[0], offs[:1]

    def correlateScan(self, scan_points_or_image, yaws, centre_xy, field_or_pyramid, field_cfg, corr_cfg, detect_cfg=None):
        """One observed scan searched over a WIDE window around a coarse candidate (a hit of localize): every yaw of `yaws` (radians) and
        every whole-cell offset |dx| <= half_x, |dy| <= half_y (corr_cfg: native.corr_config) of the scan anchored at centre_xy, against a
        field of buildLikelihoodField [height][width] or its pyramid of native.Context.field_pyramid [levels + 1 or more][height][width]
        (a field's pyramid is built for the call) -> (a native.CORR_DTYPE record, (x, y, yaw)).  The record holds the winner (rot indexes
        yaws; dx, dy in cells), its sum_d2 / n_in / n_hit as scorePoses counts them, U and the bounds evaluated and kept per level; the
        pose is the winner's metric pose (centre + (dx, dy) * cell, yaws[rot]): the start for refinePoses.  A min-pyramid of the field
        prunes the window exactly: levels = 0 searches every node and gives the same record apart from the counts.  The scan is a
        POINT_DTYPE cloud or a mono8 polar image, as in scorePoses.
        Convention: an anchor state (cos yaw, sin yaw, x, y) maps the scan's sensor frame into the map frame."""
        self._push()
        scan, _ = self._scan_or_image(scan_points_or_image, detect_cfg)
        g = native._field_cfg(field_cfg)
        yaw = np.atleast_1d(np.asarray(yaws, np.float64))
        cx, cy = (float(v) for v in centre_xy)
        if yaw.ndim != 1 or not 1 <= len(yaw) <= native.CORR_MAX_ROT or not np.all(np.isfinite(yaw)) or not (np.isfinite(cx) and np.isfinite(cy)):
            raise ValueError("yaws must be 1..%d finite angles and centre_xy two finite numbers" % native.CORR_MAX_ROT)
        k = native._corr_cfg(corr_cfg, len(yaw))
        rot = native.se2_states(yaw, cx, cy).astype(np.float32)
        f = np.asarray(field_or_pyramid)
        pyramid = f if f.ndim == 3 else self._ctx.field_pyramid(f, g, k.levels)
        rec = self._ctx.correlate_scan(scan, rot, pyramid, g, k)
        return rec, (cx + int(rec["dx"]) * g.cell, cy + int(rec["dy"]) * g.cell, float(yaw[int(rec["rot"])]))

    # ---- occupancy mapping (rr_occupancy.hip): posed scans fused into an evidence grid, and the byte map the likelihood field takes
    def buildOccupancyMap(self, clouds, states, grid, l_hit=3, l_free=2, margin_bins=None, max_free_bin=None, evidence=None):
        """n point clouds (POINT_DTYPE arrays as toPointCloud / simulatePointClouds return them: sorted by column, then bin) under their
        states float64 [n][4] (None: the identity) on `grid` (native.field_config; max_dist and gate are not used) -> (evidence int32
        [height][width], map uint8 [height][width]).  Every detection adds l_hit to its cell; every cell a scan saw to be empty -- nearer
        than the first detection of its azimuth less margin_bins, and nearer than max_free_bin -- loses l_free; the map is
        clamp(128 + evidence, 0, 255): 128 unknown, below it free, above it occupied, so distance_field(map, grid, threshold=129) is
        the likelihood field of the fused map.  margin_bins None: ceil(0.71 * cell / resolution), half a cell's diagonal, so that a
        wall's own cell is not swept free; max_free_bin None: n_cells.  evidence: an earlier call's, to accumulate into (not modified).
        The offsets of each cloud are rebuilt from its points' columns.
        Convention: a state (c, s, tx, ty) maps a cloud's sensor frame into the map frame, q = R p + t; a keyframe's state is the planar
        part of its pose, (cos yaw, sin yaw, x, y)."""
        self._push()
        n_cells = self.m_cfg.n_cells
        g = native._grid_cfg(grid)
        if isinstance(clouds, np.ndarray) and clouds.ndim == 1:
            clouds = [clouds]
        pts = [np.asarray(c) for c in clouds]
        if not pts or any(p.dtype != native.POINT_DTYPE or p.ndim != 1 for p in pts):
            raise ValueError("clouds must be a non-empty list of %ss" % native._A_CLOUD)
        offs = np.zeros((len(pts), N_ANGLES + 1), np.uint32)
        for f, p in enumerate(pts):
            col = p["column"].astype(np.int64)
            if len(col) and (col.max() >= N_ANGLES or np.any(np.diff(col) < 0)):
                raise ValueError("cloud %d is not sorted by column, or names a column past %d" % (f, N_ANGLES - 1))
            offs[f, 1:] = np.cumsum(np.bincount(col, minlength=N_ANGLES))
        if margin_bins is None:
            margin_bins = min(n_cells, int(np.ceil(0.71 * g.cell / self.m_cfg.resolution)))
        o = native.occupancy_config(l_hit, l_free, margin_bins, n_cells if max_free_bin is None else max_free_bin, n_cells)
        ev = self._ctx.occupancy_update(pts, offs, g, o, states, evidence)
        return ev, self._ctx.occupancy_map(ev, g)

    # ---- particle filter step (rr_filter.hip): score, resample and move one particle set that stays in HBM
    @staticmethod
    def effectiveSampleSize(summary):
        """total_weight^2 / sum_w2 of a FILTER_SUMMARY_DTYPE record: how many particles carry the weight (0.0 when every weight is 0)"""
        w, w2 = int(summary["total_weight"]), int(summary["sum_w2"])
        return w * w / w2 if w2 else 0.0

    def filterStep(self, scan, particles, field, field_cfg, table, filter_cfg, increment=None, n_eff_floor=None, prev_summary=None):
        """One step of a particle filter on one stream, nothing but the 32-byte summary leaving HBM: rr_score_poses_device scores the
        particles against the field, rr_filter_resample_device turns the records into weights through `table`
        (native.filter_weight_table) and draws the ancestors systematically, rr_filter_move_device moves the survivors by the odometry
        `increment` (Dc, Ds, dx, dy) in the sensor frame (None: none) plus the diffusion of filter_cfg (native.filter_config; give every
        step its own `step`, and a `phase` of the caller's choice).
        scan: a POINT_DTYPE cloud; particles: float32 [n][4] = (c, s, tx, ty), each the scan's sensor frame into the map frame, a torch
        tensor on this context's device (it is not modified) or anything numpy takes; field: the uint16 field of buildLikelihoodField,
        numpy or a torch int16 tensor on the device; table: uint16 [n_table], numpy or a torch int16 tensor on the device.
        Returns (the moved particles, a float32 [n][4] tensor on the device, the FILTER_SUMMARY_DTYPE record of the weights that were
        drawn from).  n_eff_floor: the caller's resampling rule, decided on the host from prev_summary, the summary the PREVIOUS step
        returned -- if its effective sample size is at least n_eff_floor, this step keeps every particle (the move runs without
        ancestors); the device never branches on it, and the summary is computed either way."""
        import torch
        self._push()
        g, f = native._field_cfg(field_cfg), native._filter_cfg(filter_cfg)
        inc = native._increment(increment)
        dev = torch.device("cuda", self._ctx.device)
        pts = native._scan(np.ascontiguousarray(scan), 1, "the scan")
        keep_all = n_eff_floor is not None and prev_summary is not None and self.effectiveSampleSize(prev_summary) >= float(n_eff_floor)
        n = len(particles)
        if not 1 <= n <= native.FILTER_MAX_N:
            raise ValueError("1..%d particles, got %d" % (native.FILTER_MAX_N, n))
        if not isinstance(particles, torch.Tensor) and np.asarray(particles).dtype == np.uint16:
            # uint16 states: read as numbers by castMap and refinePoses, always refused here, as words that travel as int16
            raise ValueError("particles must have shape %s and float32 elements, got %s torch.int16" % ((n, 4), np.shape(particles)))
        stream = torch.cuda.Stream(device=dev)
        s = stream.cuda_stream
        torch.cuda.current_stream(dev).synchronize()      # the caller's tensors were made on its own stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            st = self._on_device(particles, np.float32, (n, 4), "particles")
            d_field = self._on_device(field, np.int16, (g.height, g.width), "field")
            d_table = self._on_device(table, np.int16, (f.n_table,), "table")
            d_pts = torch.from_numpy(pts.view(np.uint8).copy()).to(dev)
            d_count = torch.tensor([len(pts)], dtype=torch.int32, device=dev)
            recs = torch.empty((n, 2), dtype=torch.int64, device=dev)
            cum = torch.empty(n, dtype=torch.int64, device=dev)
            anc = torch.empty(n, dtype=torch.int32, device=dev)
            summary = torch.empty(4, dtype=torch.int64, device=dev)
            out = torch.empty((n, 4), dtype=torch.float32, device=dev)
            self._ctx.score_poses_device(d_pts.data_ptr(), d_count.data_ptr(), len(pts), st.data_ptr(), n, d_field.data_ptr(), g, recs.data_ptr(), s)
            self._ctx.filter_resample_device(recs.data_ptr(), n, d_table.data_ptr(), n, f, cum.data_ptr(), anc.data_ptr(), summary.data_ptr(), s)
            self._ctx.filter_move_device(st.data_ptr(), n, None if keep_all else anc.data_ptr(), n, inc, f, out.data_ptr(), s)
            home = summary.cpu().numpy().view(native.FILTER_SUMMARY_DTYPE)[0].copy()
        self._ctx.synchronize(s)
        self.m_filter = dict(recs=recs, cum=cum, ancestors=anc)      # the step's intermediates, on the device, for who wants to look
        return out, home

    # ---- map refinement (rr_refine.hip): the nearest-cell table of a grid map, and one scan refined against it from many states
    def _on_device(self, x, dtype, shape, what):
        """a tensor, or an array numpy takes, -> a contiguous tensor on the context's device; torch lacks uint16 and uint32 arithmetic, so
        such words travel as int16 and int32"""
        import torch
        dev = torch.device("cuda", self._ctx.device)
        if not isinstance(x, torch.Tensor):
            a = np.ascontiguousarray(x)
            signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}.get(a.dtype)
            a = a.view(signed) if signed is not None and np.dtype(signed) == np.dtype(dtype) else np.ascontiguousarray(a, dtype)
            x = torch.from_numpy(a.copy())
        if tuple(x.shape) != shape or x.element_size() != np.dtype(dtype).itemsize or x.is_floating_point() != (np.dtype(dtype).kind == "f"):
            raise ValueError("%s must have shape %s and %s elements, got %s %s" % (what, shape, np.dtype(dtype), tuple(x.shape), x.dtype))
        return x.to(dev).contiguous()

    def buildNearestField(self, occ, field_cfg, threshold=1):
        """An occupancy map uint8 [height][width] -- a grid of rasterize_points at threshold 1, a map of buildOccupancyMap at 129; numpy or
        a torch tensor on the device -- -> its nearest-cell table, an int32 [height][width] tensor on the device (rr_nearest_field_device;
        the words are uint32: jy * width + jx of the nearest occupied cell, native.NEAREST_NONE = -1 as int32 where none lies within
        max_dist).  The table stays in HBM for refinePoses."""
        import torch
        self._push()
        g, th = native._field_cfg(field_cfg), native._int_in(threshold, 1, 255, "threshold")
        dev = torch.device("cuda", self._ctx.device)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.current_stream(dev).synchronize()      # the caller's tensor was made on its own stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            d_occ = self._on_device(occ, np.uint8, (g.height, g.width), "occ")
            table = torch.empty((g.height, g.width), dtype=torch.int32, device=dev)
            self._ctx.nearest_field_device(d_occ.data_ptr(), g, table.data_ptr(), th, stream.cuda_stream)
        self._ctx.synchronize(stream.cuda_stream)
        return table

    @staticmethod
    def refineRecords(recs):
        """the float64 [n][6] tensor of refinePoses -> native.ICP_DTYPE [n] on the host (c, s, tx, ty, sse, n_matched, flags)"""
        return recs.detach().cpu().contiguous().numpy().view(np.uint8).reshape(-1).view(native.ICP_DTYPE).copy()

    def refinePoses(self, scan, states, nearest, field_cfg, iterations=10):
        """ONE observed scan refined against the map from every state of `states` at once: point-to-point ICP against the nearest-cell table
        of buildNearestField, all iterations in one launch (rr_refine_poses_device), nothing leaving HBM.
        scan: a POINT_DTYPE cloud; states: [n][4] = (c, s, tx, ty), each the scan's sensor frame into the map frame -- float32 as
        native.pose_lattice and filterStep give them, or float64; numpy or a torch tensor on the device; float32 is widened to float64 on
        the device; nearest: the int32 tensor of buildNearestField (or a uint32 array); field_cfg.gate is the match gate in cells.
        Returns a float64 [n][6] tensor on the device, one 48-byte rr_icp_rec per row: columns 0..3 are the refined state, which
        rasterize_points and occupancy_update take as it is; refineRecords() reads all of it (sse, n_matched, flags) on the host."""
        import torch
        self._push()
        g, it = native._refine_cfg(field_cfg), native._int_in(iterations, 0, 64, "iterations")
        dev = torch.device("cuda", self._ctx.device)
        pts = native._scan(np.ascontiguousarray(scan), 1, "the scan")
        n = len(states)
        if not 1 <= n <= native.FIELD_MAX_HYP:
            raise ValueError("1..%d states, got %d" % (native.FIELD_MAX_HYP, n))
        wide = states.dtype == torch.float64 if isinstance(states, torch.Tensor) else np.asarray(states).dtype == np.float64
        stream = torch.cuda.Stream(device=dev)
        s = stream.cuda_stream
        torch.cuda.current_stream(dev).synchronize()      # the caller's tensors were made on its own stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            st = self._on_device(states, np.float64 if wide else np.float32, (n, 4), "states").to(torch.float64).contiguous()
            d_near = self._on_device(nearest, np.int32, (g.height, g.width), "nearest")
            d_pts = torch.from_numpy(pts.view(np.uint8).copy()).to(dev)
            d_count = torch.tensor([len(pts)], dtype=torch.int32, device=dev)
            recs = torch.empty((n, 6), dtype=torch.float64, device=dev)
            self._ctx.refine_poses_device(d_pts.data_ptr(), d_count.data_ptr(), len(pts), st.data_ptr(), n, d_near.data_ptr(), g, recs.data_ptr(), it, s)
        self._ctx.synchronize(s)
        return recs

    # ---- beam model (rr_cast.hip): the map cast at pose hypotheses, and a scan's rays scored against it
    def _scan_with_offsets(self, scan_points_or_image, detect_cfg):
        """a POINT_DTYPE cloud (sorted by column, then bin; its offsets are rebuilt from the columns) or a mono8 polar image, which is
        detected first -> ([cloud], offsets uint32 [1][401])"""
        scan, offs = self._scan_or_image(scan_points_or_image, detect_cfg)
        if offs is not None:
            return [scan], offs
        scan = native._scan(scan, None, "the scan")
        col = scan["column"].astype(np.int64)
        if len(col) and (col.max() >= N_ANGLES or np.any(np.diff(col) < 0)):
            raise ValueError("the scan is not sorted by column, or names a column past %d" % (N_ANGLES - 1))
        offs = np.zeros((1, N_ANGLES + 1), np.uint32)
        offs[0, 1:] = np.cumsum(np.bincount(col, minlength=N_ANGLES))
        return [scan], offs

    def scanProfile(self, scan_points_or_image, detect_cfg=None):
        """One observed scan -> uint16 [400]: per azimuth INDEX the bin of its first detection, n_cells where it has none
        (rr_scan_profile).  The scan is a POINT_DTYPE cloud or a mono8 polar image [n_cells][400], as scorePoses takes it."""
        self._push()
        pts, offs = self._scan_with_offsets(scan_points_or_image, detect_cfg)
        return self._ctx.scan_profile(pts, offs)[0]

    def beamDirections(self):
        """float32 [400][2]: (cos, sin) of every azimuth index under the current config (native.beam_directions)"""
        self._push()
        return native.beam_directions(self._ctx._rrcfg)

    def castMap(self, states, field, field_cfg, beam_cfg):
        """The expected scan of the map at each state: float32 states [n][4] = (c, s, tx, ty), n <= 65535 (native.pose_lattice makes them),
        each the sensor frame into the map frame, cast through the uint16 field of buildLikelihoodField (or of distance_field on a map of
        buildOccupancyMap at threshold 129) -> an int16 [n][400] tensor on the device whose words are uint16: per azimuth index the first
        sampled bin whose cell is occupied, beam_cfg's bin_end where the ray meets nothing (rr_cast_map_device; beam_cfg:
        native.beam_config or a dict of its arguments).  states and field: numpy or torch tensors on the device."""
        import torch
        self._push()
        g, b = native._cast_cfg(field_cfg), self._ctx._beam_cfg(beam_cfg)
        n = len(states)
        if not 1 <= n <= native.CAST_MAX_HYP:
            raise ValueError("1..%d states, got %d" % (native.CAST_MAX_HYP, n))
        dev = torch.device("cuda", self._ctx.device)
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.current_stream(dev).synchronize()      # the caller's tensors were made on its own stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            st = self._on_device(states, np.float32, (n, 4), "states")
            d_field = self._on_device(field, np.int16, (g.height, g.width), "field")
            d_dirs = torch.from_numpy(native.beam_directions(self._ctx._rrcfg)).to(dev)
            ranges = torch.empty((n, N_ANGLES), dtype=torch.int16, device=dev)
            self._ctx.cast_map_device(st.data_ptr(), n, d_dirs.data_ptr(), d_field.data_ptr(), g, b, ranges.data_ptr(), stream.cuda_stream)
        self._ctx.synchronize(stream.cuda_stream)
        return ranges

    def scoreBeams(self, scan_points_or_image, states, field, field_cfg, beam_cfg, detect_cfg=None):
        """One observed scan against float32 states [n][4] and the field of a map -> native.BEAM_DTYPE [n]: per state the azimuths whose
        measured first detection agrees with the range the map predicts (n_agree), stops short of it (n_short), lies beyond it or is
        missing where the map has a wall (n_through), and sum_abs of the clipped differences; more n_agree is better.  The scan is a
        POINT_DTYPE cloud or a mono8 polar image, as scorePoses takes it; its profile is scanProfile's.
        Convention: a hypothesis state (c, s, tx, ty) maps the scan's sensor frame into the map frame."""
        self._push()
        pts, offs = self._scan_with_offsets(scan_points_or_image, detect_cfg)
        first = self._ctx.scan_profile(pts, offs)[0]
        return self._ctx.score_beams(first, states, native.beam_directions(self._ctx._rrcfg), field, field_cfg, beam_cfg)

    # ---- mesh maps (rr_slice.hip): the loaded mesh itself as the grid map, no scans in between
    def buildMeshMap(self, field_cfg, z_lo, z_hi, skip_objects=(), with_objects=False, occ=None):
        """The scene's triangles as a prior map: uint8 [height][width], a 1 in every cell of field_cfg's grid that some triangle -- every
        face's rest corners moved by its object's current pose (setObjectPoses) -- touches inside the height band [z_lo, z_hi] (metres,
        map frame; around the sensor plane), 0 elsewhere (rr_slice_mesh).  Geometry only: no occlusion, no materials, no noise.
        skip_objects: object ids left out entirely, e.g. the parked and moving objects of a dynamic scene.  with_objects: also the uint32
        plane of the smallest object id per cell (native.OBJECT_NONE where nothing marks it), a semantic map through object_materials.
        occ: a map to accumulate into (a copy of it is returned): another band, or a grid of rasterize_points.
        Returns occ, or (occ, objects), as numpy arrays.
        The chain: buildMeshMap -> the transform of buildLikelihoodField (Context.distance_field at threshold 1) for scorePoses, castMap
        and scoreBeams; -> buildNearestField for refinePoses."""
        out = self._ctx.slice_mesh(native.slice_config(z_lo, z_hi), field_cfg, skip_objects, with_objects, occ)
        return out

    # ---- connected components (rr_components.hip): the returns of polar images as clusters, the occupied cells of a grid map as segments
    def _label(self, planes, cfg, labels, clean):
        """numpy planes: the host form; a torch tensor on the device: the device form on a stream of its own, nothing leaving HBM"""
        try:
            import torch
            on_device = isinstance(planes, torch.Tensor)
        except ImportError:
            on_device = False
        if not on_device:
            return self._ctx.label_components(planes, cfg, labels, clean)
        dev = planes.device
        stream = torch.cuda.Stream(device=dev)            # an explicit stream, as simulatePointClouds
        torch.cuda.current_stream(dev).synchronize()      # the caller's tensor was made on its own stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            out = self._ctx.label_components_tensors(planes, cfg, labels, clean, stream.cuda_stream)
        self._ctx.synchronize(stream.cuda_stream)
        del out["scratch"]
        return out

    def clusterImages(self, imgs_u8, threshold, connectivity=8, min_pixels=1, max_components=4096):
        """Polar images uint8 [n][n_cells][400] (or one image), real or simulated -> their returns grouped into clusters: the connected
        components of the pixels >= threshold (rr_label_components), rows range bins and columns azimuths.  A polar image is a cylinder, so
        the column axis wraps: a cluster across the first and last column is one (its record carries native.COMP_SEAM, and col_hi_min ..
        399, 0 .. col_lo_max is its arc); the scroll of the image does not matter.  Clusters below min_pixels are dropped.
        numpy images take the host form and return numpy; a torch uint8 tensor on the context's device takes the device form on a stream of
        its own and returns tensors that never leave HBM (native.Context.label_components_tensors; component_records brings records home).
        Returns a dict: labels [n][n_cells][400] (the smallest linear index of the pixel's cluster, native.LABEL_NONE elsewhere), comps (per
        image the first max_components COMPONENT_DTYPE records in ascending root order) and counts [n][2] = (kept, dropped).
        Sparse CFAR points rarely touch: dilate first where gaps are to be bridged."""
        cfg = native.components_config(self.m_cfg.n_cells, N_ANGLES, threshold, connectivity, True, min_pixels, max_components)
        return self._label(imgs_u8, cfg, True, False)

    def segmentMap(self, occ_u8, field_cfg, threshold, min_cells=1, connectivity=8):
        """A grid map uint8 [height][width] of field_cfg's grid (a grid of rasterize_points or buildMeshMap at threshold 1, a map of
        buildOccupancyMap at 129; numpy, or a torch tensor on the device) -> (the cleaned map, the records): the occupied cells grouped into
        segments without wrap, segments below min_cells dropped -- a three-cell phantom that survived the evidence threshold is no zero of
        the distance field any more.  The cleaned map keeps the input's bytes under every kept cell and is 0 elsewhere, so it goes on to
        distance_field / buildNearestField / castMap at the same threshold.  The records: COMPONENT_DTYPE, every kept segment in ascending
        root order (the map is labelled once for the count, then with room for every record, when there are more than 4096)."""
        g = native._field_cfg(field_cfg)
        cfg = native.components_config(g.height, g.width, threshold, connectivity, False, min_cells, 4096)
        out = self._label(occ_u8, cfg, False, True)
        kept = int(native.Context.component_counts(out["counts"])[0, 0])
        if kept > cfg.max_components:
            cfg.max_components = kept
            out = self._label(occ_u8, cfg, False, True)
        recs = out["comps"] if isinstance(out["comps"], list) else native.Context.component_records(out["comps"], out["counts"])
        return out["clean"][0], recs[0]

    # ---- place recognition (rr_place.hip): a database of yaw-invariant ring/sector descriptors, and a scan looked up in it
    def buildPlaceDatabase(self, poses, place_cfg, on_device=False):
        """any number of [n][7] poses, worked through 64 at a time -> their descriptors uint8 [n][R][S] (native.Context._place_cfg
        says what place_cfg may be); no image leaves the GPU.  on_device: the database stays in HBM, as a torch tensor."""
        self._push()
        p = native.object_poses_array(poses)
        cfg = self._ctx._place_cfg(place_cfg)
        self._place_cfg = cfg
        if not on_device:
            if len(p) == 0:
                return np.zeros((0, cfg.n_rings, cfg.n_sectors), np.uint8)
            return np.concatenate([self._ctx.simulate_batch_describe(p[at:at + 64], cfg) for at in range(0, len(p), 64)])
        import torch
        dev = torch.device("cuda", self._ctx.device)
        stream = torch.cuda.Stream(device=dev)      # an explicit stream, as simulatePointClouds
        s = stream.cuda_stream
        with torch.cuda.device(dev), torch.cuda.stream(stream):
            db = torch.empty((len(p), cfg.n_rings, cfg.n_sectors), dtype=torch.uint8, device=dev)
            imgs = torch.empty((min(64, max(1, len(p))), self.m_cfg.n_cells, N_ANGLES), dtype=torch.uint8, device=dev)
            for at in range(0, len(p), 64):
                chunk = p[at:at + 64]
                self._ctx.simulate_batch_device(chunk, imgs.data_ptr(), s)
                self._ctx.describe_images_device(imgs.data_ptr(), len(chunk), cfg, db[at:].data_ptr(), s)
        self._ctx.synchronize(s)
        return db

    def localize(self, real_polar, database, poses, top_k, place_cfg=None):
        """ONE real polar image looked up in `database` (buildPlaceDatabase's, host array or HBM tensor) -> (a native.PLACE_DTYPE
        array [top_k], ranked by (sse, index); float32 [top_k][7]: per hit the database pose turned by the shift's yaw).  place_cfg
        None: the one of the last buildPlaceDatabase.  The shift s moves the REAL scan's sectors, so by the rule registerPose uses for an
        azimuth shift the real pose turned by -s * (n_angles / S) * theta_inc about the sensor's z axis is the database pose; the
        database pose is therefore turned by +s * (n_angles / S) * theta_inc.  Exact only when S divides n_angles -- otherwise
        sector widths differ by one column and the yaw is approximate."""
        self._push()
        cfg = self._ctx._place_cfg(place_cfg if place_cfg is not None else getattr(self, "_place_cfg", None) or tuple(database.shape[1:]))
        if tuple(database.shape[1:]) != (cfg.n_rings, cfg.n_sectors):
            raise ValueError("the database holds descriptors %s, the config says %s" % (tuple(database.shape[1:]), (cfg.n_rings, cfg.n_sectors)))
        p = native.object_poses_array(poses)
        if len(p) != len(database):
            raise ValueError("%d poses for %d database entries" % (len(p), len(database)))
        q = self._ctx.describe_images(self._polar(real_polar), cfg)
        if isinstance(database, np.ndarray):
            rec = self._ctx.match_descriptors(q, database, top_k)[0]
        else:
            import torch
            d_q = torch.from_numpy(q).to(database.device)
            rec = self._ctx.match_descriptors_device(d_q.data_ptr(), 1, database.data_ptr(), len(database), cfg.n_rings, cfg.n_sectors, top_k)[0]
        S = cfg.n_sectors
        s = rec["shift"].astype(np.int64)
        s = np.where(2 * s > S, s - S, s)
        half = 0.5 * s * (N_ANGLES / S) * float(self._ctx._rrcfg.theta_inc)
        bz, bw = np.sin(half), np.cos(half)                           # q * (0, 0, bz, bw): a turn in the sensor's own frame
        hit = p[rec["index"]].astype(np.float64)
        ax, ay, az, aw = hit[:, 0].copy(), hit[:, 1].copy(), hit[:, 2].copy(), hit[:, 3].copy()
        hit[:, 0], hit[:, 1] = ax * bw + ay * bz, ay * bw - ax * bz
        hit[:, 2], hit[:, 3] = aw * bz + az * bw, aw * bw - az * bz
        return rec, hit.astype(np.float32)

    def _push(self):
        if self._dirty_cfg:
            cfg = self.m_cfg.copy(n_reflections=self.m_params.model.n_reflections)
            self._ctx.set_config(cfg, N_ANGLES, wave_energy_threshold=self.m_wave_energy_threshold)
            self._dirty_cfg = False
        if self._dirty_mat:
            self._ctx.set_materials(self.m_params.materials, self.m_object_materials, self.m_material_id_air)
            self._dirty_mat = False
        if self.m_resample:     # RadarCPU.cpp:136-145
            self.m_waves_start = beams.sample_cone_local_rad(     # model.beam_width: radians, what the C++ twin passes
                self.m_params.model.beam_width, self.m_params.model.n_samples, self.m_cfg.beam_sample_dist,
                self.m_cfg.beam_sample_dist_normal_p_in_cone, seed=self._beam_seed)
            self._ctx.set_beam_samples(self.m_waves_start)
            self.m_resample = False

    # -- the seam: Radar.hpp:64 / RadarCPU.cpp:30-564
    def simulate(self, stamp=0.0, want_f32=False):
        if not self.updateTsm():
            print("Couldn't get Transform between sensor and map. Skipping...")   # RadarCPU.cpp:131
            return None
        self._push()
        u8, f32, stats = self._ctx.simulate(self.Tsm_last, 0, N_ANGLES, want_f32=want_f32)
        msg = Image(header=Header(stamp=stamp, frame_id=self.m_sensor_frame),
                    height=u8.shape[0], width=u8.shape[1], encoding="mono8", step=u8.shape[1], data=u8)
        self.last_f32 = f32
        self.last_stats = stats
        return msg

    def simulate_provenance(self, pose=None, echo_stride=None):
        """What the image is made of (rr_simulate_provenance): the frame at `pose` ([7], default: the current Tsm) ->
        (image u8 [n_cells][400], labels uint32, faces uint32, echoes native.ECHO_SRC_DTYPE [400][echo_stride], counts uint32 [400]).
        labels / faces hold, per pixel, the info word and the face of the echo with the largest single term in that range bin
        (native.LABEL_NONE: no echo reaches it); echoes is every azimuth's ordered echo stream, indexed by azimuth, counts its
        true lengths.  unpack_info() splits an info word; a ghost mask is `pass > 0`."""
        if pose is None:
            if not self.updateTsm():
                print("Couldn't get Transform between sensor and map. Skipping...")
                return None
            pose = self.Tsm_last
        self._push()
        return self._ctx.simulate_provenance(pose, echo_stride=echo_stride)

    def simulate_paths(self, pose=None, wave_stride=None, map_frame=False):
        """By which route the waves travelled (rr_simulate_paths): the frame at `pose` ([7], default: the current Tsm) ->
        (image u8 [n_cells][400], records native.WAVE_DTYPE [400][wave_stride], counts uint32 [400], pass_counts uint32 [400][16]).
        records holds every azimuth's list of ray-cast waves (misses included), indexed by azimuth; counts its true lengths.
        wave_stride None: one run to learn the counts, then the run that fills the rows.  map_frame: o / d in the map frame.
        unpack_wave_info / hit_points / path_to_wave / path_to_echo read one azimuth's row, records[a][:counts[a]]."""
        if pose is None:
            if not self.updateTsm():
                print("Couldn't get Transform between sensor and map. Skipping...")
                return None
            pose = self.Tsm_last
        self._push()
        return self._ctx.simulate_paths(pose, wave_stride=wave_stride, map_frame=map_frame)

    def simulate_doppler(self, pose=None, sensor_vel=None, gain=0.0, echo_stride=None, want_f32=False, want_vel_img=True):
        """The frame as an FMCW sweep sees a moving scene (rr_simulate_doppler): every echo is drawn gain * v_r metres away from where the
        mesh says it is, v_r its range rate under the objects' twists (set_object_twists on the context) and the sensor's velocity
        sensor_vel ([3], map frame, m/s; default 0).  pose [7], default: the current Tsm.  -> (image u8 [n_cells][400], f32 image or None,
        v_r float32 [400][echo_stride], shifted cells int32 [400][echo_stride] (-1: dropped), counts uint32 [400], velocity image float32
        [n_cells][400] or None (NaN where no echo reaches the bin)); the rows are indexed like simulate_provenance's echo stream."""
        if pose is None:
            if not self.updateTsm():
                print("Couldn't get Transform between sensor and map. Skipping...")
                return None
            pose = self.Tsm_last
        self._push()
        return self._ctx.simulate_doppler(pose, sensor_vel=sensor_vel, gain=gain, echo_stride=echo_stride, want_f32=want_f32, want_vel_img=want_vel_img)

    def _batch(self, poses, sweeps, stamp):
        """Offline generation (the twin of integration/.../RadarHIP.cpp: simulateBatch / simulateSweeps): one image per pose,
        up to 64 poses per set of launches, delivered to page-locked host memory (rr_simulate_batch_host_async)."""
        self._push()
        out = []
        poses = np.ascontiguousarray(poses, np.float32)
        n_total = len(poses)
        for at in range(0, n_total, 64):
            chunk = poses[at:at + 64]
            if sweeps:         # chunk: [n][n_angles][7] -- table k = the per-azimuth poses of frame k (RadarCPU.cpp:190-196)
                self._ctx.set_motion_poses(chunk.reshape(-1, 7))
                first = np.ascontiguousarray(chunk[:, 0, :])
            else:
                self._ctx.set_motion_poses(None)
                first = chunk
            h = native.HostImages((len(chunk), self.m_cfg.n_cells, N_ANGLES))
            try:
                self._ctx.simulate_batch_host_async(first, h.ptr)
                self._ctx.wait_host(h.ptr)
                for k in range(len(chunk)):
                    u8 = h.array[k].copy()
                    out.append(Image(header=Header(stamp=stamp, frame_id=self.m_sensor_frame), height=u8.shape[0], width=u8.shape[1],
                                     encoding="mono8", step=u8.shape[1], data=u8))
            finally:
                h.close()
        self._ctx.set_motion_poses(self._motion if getattr(self, "_motion", None) is not None else None)
        return out

    def simulateBatch(self, poses, stamp=0.0):
        """[n][7] poses -> n Images (one set of launches per 64 poses)."""
        return self._batch(np.asarray(poses, np.float32).reshape(-1, 7), False, stamp)

    def simulateSweeps(self, sweeps, stamp=0.0):
        """include_motion: [n][400][7] per-azimuth pose tables -> n Images, one table per frame of a batch."""
        return self._batch(np.asarray(sweeps, np.float32).reshape(-1, N_ANGLES, 7), True, stamp)

    def simulateMaterialSets(self, sets, stamp=0.0):
        """The gen_radar_image action of the optimisation loop (action/GenRadarImage.action,
        scripts/radaray_opti.py:170-200), batched: `sets` is a list of material lists (each as long
        as loadParams() gave); returns one mono8 Image per set for the current pose, one call."""
        if not self.updateTsm():
            print("Couldn't get Transform between sensor and map. Skipping...")
            return []
        self._push()
        n_mat = len(self.m_params.materials)
        if any(len(x) != n_mat for x in sets):
            raise ValueError("every material set needs %d entries" % n_mat)
        arr = [[m.astuple() for m in x] for x in sets]
        imgs = self._ctx.simulate_material_sets(self.Tsm_last, arr)
        return [Image(header=Header(stamp=stamp, frame_id=self.m_sensor_frame), height=u8.shape[0], width=u8.shape[1],
                      encoding="mono8", step=u8.shape[1], data=u8) for u8 in imgs]

    def simulateParamSets(self, sets, stamp=0.0, real=None, want_images=True, metrics=None, win_size=7):
        """The same action over the optimiser's WHOLE parameter vector (scripts/radaray_opti.py:36-113): `sets` is a list
        of RadarParams (materials + model.beam_width [rad] / n_samples / n_reflections); one rr_simulate_param_sets call.
        Beams are drawn like _push() draws them (same seed: equal widths share pass 0).  Returns (images or None,
        psnr or None) -- with `real` (mono8 [n_cells][400]) the objective values of radaray_opti.py:196.  With `metrics`
        (a native.METRIC_* mask or names) the second value is a native.METRICS_DTYPE array instead: any of the script's
        metrics as the objective (rr_simulate_param_sets_metrics)."""
        if not self.updateTsm():
            print("Couldn't get Transform between sensor and map. Skipping...")
            return None, None
        self._push()
        n_mat, nb = len(self.m_params.materials), self.m_params.model.n_samples
        ps = []
        for p in sets:
            if len(p.materials) != n_mat or p.model.n_samples != nb:
                raise ValueError("every parameter set needs %d materials and n_samples = %d" % (n_mat, nb))
            dirs = None
            if abs(p.model.beam_width - self.m_params.model.beam_width) > 1e-7:
                dirs = beams.sample_cone_local_rad(p.model.beam_width, nb, self.m_cfg.beam_sample_dist,
                                                   self.m_cfg.beam_sample_dist_normal_p_in_cone, seed=self._beam_seed)
            ps.append({"materials": [m.astuple() for m in p.materials], "beam_dirs": dirs, "n_reflections": int(p.model.n_reflections)})
        imgs, psnr = self._ctx.simulate_param_sets(self.Tsm_last, ps, n_mat, ref_u8=None if real is None else self._polar(real),
                                                   want_images=want_images, metrics=metrics, win_size=win_size)
        msgs = None if imgs is None else [
            Image(header=Header(stamp=stamp, frame_id=self.m_sensor_frame), height=u8.shape[0], width=u8.shape[1],
                  encoding="mono8", step=u8.shape[1], data=u8) for u8 in imgs]
        return msgs, psnr

    @property
    def context(self):
        return self._ctx
